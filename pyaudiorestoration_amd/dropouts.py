"""MaxMono dropout repair (dropouts_gui.MainWindow.process_max_mono, dropouts_gui.py:137-163) on the GPU.

A two-track transfer of a mono tape: for every STFT bin the louder of the two channels is kept, so a dropout in one track is
filled from the other ("max"); the twin that keeps the quieter channel is used against clicks ("min").

    y_pad = fix_length(signal, n + fft_size // 2, axis=0)
    D_L, D_R = stft(y_pad[:, 0], fft_size, hop), stft(y_pad[:, 1], fft_size, hop)        # blackmanharris, zeropad 1
    max: D = where(|D_L| > |D_R|, D_L, D_R)        min: D = where(|D_L| < |D_R|, D_L, D_R)
    y = istft(D, length=n, hop_length=hop)                                               # <stem>max.wav / <stem>min.wav, mono

On a tie, and where a magnitude is NaN, both outputs take D_R.  Here the whole chain is one launch of par_maxmono_stft_f32
(no spectrogram reaches HBM) where FUSED says so; otherwise K_stft twice, par_select_spectrum_f32 and K_istft twice, all on
the device.  The composed route decides as numpy's complex64 np.abs does on K_stft mode 0's spectra, bit for bit.  The fused
kernel decides the same except, possibly, in bins whose two magnitudes lie within a few float32 ulps of each other (its spectra
can differ from K_stft's in the last bit; include/par_hip.h states the bound): 2 bins of 2.1e8 on a 10-min file at 2048/128."""
import os

import numpy as np
import torch

from . import _dev, _lib, fourier, io_ops

WINDOW = "blackmanharris"
FFT_SIZE = 512          # dropouts_gui.py:43: the display widget's FFT size is set to its fourth entry
OVERLAP = 4             # util/widgets.py:343-345: the display widget's default overlap
SUFFIXES = ("max", "min")


def fused_supported(fft_size, hop):
    """The sizes par_maxmono_stft_f32 takes: power-of-two transforms of 16..8192 points with 1 <= hop <= n_fft whose frames and
    two overlap-add rings fit the LDS (every hop up to 4096 points; hop <= 5114 at 8192)."""
    return bool(_lib.lib().par_maxmono_stft_supported(int(fft_size), int(hop)))


FUSED_MAX_FFT = 2048
FUSED_MAX_OVERLAP = 16


def FUSED(fft_size, hop):
    """The policy: True where the fused kernel was measured faster.  On a 10-min stereo file (NOTES.md, MaxMono) it wins at
    512/64, 2048/512 and 2048/128 (overlaps 4 to 16, by 1.39 x, 1.16 x and 1.03 x: the margin shrinks as the overlap grows) and
    loses at 8192/1024.  What is not measured takes the composed route, the yardstick: 4096 points and more, and hops under
    n_fft / 16."""
    fft_size, hop = int(fft_size), int(hop)
    return fft_size <= FUSED_MAX_FFT and hop * FUSED_MAX_OVERLAP >= fft_size and fused_supported(fft_size, hop)


def _check_sizes(fft_size, hop):
    fft_size, hop = int(fft_size), int(hop)
    if fft_size < 2 or fft_size % 2 or hop < 1:
        raise ValueError(f"fft_size {fft_size} / hop {hop}: need an even fft_size >= 2 and hop >= 1")
    return fft_size, hop


def _check_channels(channels, ch):
    chans = tuple(int(c) for c in channels)
    if len(chans) != 2:
        raise ValueError(f"channels {chans}: MaxMono takes the two channels (L, R)")
    for c in chans:
        if not 0 <= c < ch:
            raise IndexError(f"channel {c} of a {ch}-channel signal")
    return chans


def _check_stereo(shape):
    if len(shape) != 2 or shape[1] != 2:
        raise ValueError(f"expects stereo input, got shape {tuple(shape)}")


def select_spectra_dev(fmL, fmR, dev=None, want_min=True):
    """Frame-major complex64 device spectrograms [frames][bins] (contiguous) -> (max, min) of the same layout (min None when not
    wanted).  One call of par_select_spectrum_f32."""
    if fmL.shape != fmR.shape or fmL.ndim != 2 or fmL.dtype != torch.complex64 or fmR.dtype != torch.complex64:
        raise ValueError(f"two complex64 spectrograms of one shape, got {tuple(fmL.shape)} {fmL.dtype} / {tuple(fmR.shape)} {fmR.dtype}")
    dev = _dev.device_index(dev if dev is not None else fmL.device)
    fmL, fmR = fmL.contiguous(), fmR.contiguous()
    out_max = torch.empty_like(fmL)
    out_min = torch.empty_like(fmL) if want_min else None
    frames, bins = fmL.shape
    if bins:
        _lib.check(_lib.lib().par_select_spectrum_f32(dev, _dev.ptr(fmL), _dev.ptr(fmR), frames, bins, 0, _dev.ptr(out_max),
                                                      _dev.ptr(out_min) if want_min else None, _dev.stream_ptr(dev)))
    return out_max, out_min


def select_spectra(DL, DR, device=None):
    """(D_max, D_min) = (where(|DL| > |DR|, DL, DR), where(|DL| < |DR|, DL, DR)) of two spectrograms of one 2-D shape, any
    orientation: numpy complex in -> numpy complex64 out, device tensors in -> device tensors out."""
    if torch.is_tensor(DL) != torch.is_tensor(DR):
        raise ValueError("both spectrograms numpy or both device tensors")
    if tuple(DL.shape) != tuple(DR.shape) or DL.ndim != 2:
        raise ValueError(f"two 2-D spectrograms of one shape, got {tuple(DL.shape)} / {tuple(DR.shape)}")
    dev = _dev.device_index(device if device is not None else (DL.device if torch.is_tensor(DL) else None))
    if torch.is_tensor(DL):
        mx, mn = select_spectra_dev(DL.to(torch.complex64), DR.to(torch.complex64), dev)
        return mx, mn
    mx, mn = select_spectra_dev(_dev.to_dev(np.asarray(DL), torch.complex64, dev), _dev.to_dev(np.asarray(DR), torch.complex64, dev), dev)
    return _dev.to_host(mx), _dev.to_host(mn)


def max_mono_dev(sig_t, fft_size=FFT_SIZE, hop=FFT_SIZE // OVERLAP, channels=(0, 1), window_name=WINDOW, fused=None, dev=None, out=None):
    """Device form of max_mono: sig_t float32 (n, ch >= 2) device tensor, `channels` its L and R -> (y_max, y_min), float32 (n,)
    device tensors: the two columns of one (n, 2) tensor (out: such a tensor to write to).  fused: None lets FUSED pick by
    size, True asks for par_maxmono_stft_f32 (ParUnsupported for the sizes it does not take), False forces the composed route
    (K_stft twice, par_select_spectrum_f32, K_istft twice; the tests' reference for the fused kernel)."""
    fft_size, hop = _check_sizes(fft_size, hop)
    if sig_t.ndim != 2 or sig_t.shape[1] < 2:
        raise ValueError(f"expects an (n, 2+) signal, got shape {tuple(sig_t.shape)}")
    n, ch = sig_t.shape
    if n < 1:
        raise ValueError("empty signal")
    cl, cr = _check_channels(channels, ch)
    dev = _dev.device_index(dev if dev is not None else sig_t.device)
    sig_t = _dev.to_dev(sig_t, torch.float32, dev)
    window_t = fourier.window_dev(window_name, fft_size, dev)
    if out is None:
        out = _dev.empty((n, 2), torch.float32, dev)
    if tuple(out.shape) != (n, 2) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out: a contiguous float32 (n, 2) tensor")
    use_fused = FUSED(fft_size, hop) if fused is None else fused
    if use_fused:
        flat = sig_t.reshape(-1)
        oflat = out.reshape(-1)
        _lib.check(_lib.lib().par_maxmono_stft_f32(dev, _dev.ptr(flat[cl:]), _dev.ptr(flat[cr:]), n, ch, fft_size, hop, _dev.ptr(window_t),
                                                   _dev.ptr(oflat), 2, _dev.ptr(oflat[1:]), 2, _dev.stream_ptr(dev)))
        return out[:, 0], out[:, 1]
    half = fft_size // 2
    fms = []
    for c in (cl, cr):
        xpad = torch.zeros(n + half, dtype=torch.float32, device=f"cuda:{dev}")        # fourier.fix_length(sig, n + n_fft // 2)
        xpad[:n] = sig_t[:, c]
        fms.append(fourier.stft_dev(xpad, fft_size, hop, window_t, 1, 0, dev=dev).T)     # [frames][bins]
    sel = select_spectra_dev(fms[0], fms[1], dev)
    del fms
    for k, fm in enumerate(sel):
        out[:, k] = fourier.istft_dev(fm.T, hop, window_t, length=n, dev=dev)
    return out[:, 0], out[:, 1]


def max_mono(signal, sr=None, fft_size=FFT_SIZE, hop=FFT_SIZE // OVERLAP, channels=(0, 1), window_name=WINDOW, fused=None, device=None):
    """process_max_mono on an (n, 2) float32 signal: (y_max, y_min), float32 (n,) each -- numpy for numpy input, device tensors
    for a tensor.  Anything but stereo raises ValueError (the reference prints "expects stereo input" and skips the file).  sr is
    not used (the transform does not depend on it); it is taken for the call shape of the other tools."""
    fft_size, hop = _check_sizes(fft_size, hop)
    _check_stereo(signal.shape)
    _check_channels(channels, signal.shape[1])
    dev = _dev.device_index(device if device is not None else (signal.device if torch.is_tensor(signal) else None))
    was_tensor = torch.is_tensor(signal)
    sig_t = _dev.to_dev(signal, torch.float32, dev)                                      # both channels go up once
    out = _dev.empty((sig_t.shape[0], 2), torch.float32, dev)
    y_max, y_min = max_mono_dev(sig_t, fft_size, hop, channels, window_name, fused, dev, out)
    if was_tensor:
        return y_max, y_min
    both = _dev.to_host(out)                                                             # ... and both results come down once
    return np.ascontiguousarray(both[:, 0]), np.ascontiguousarray(both[:, 1])


def output_paths(path):
    """The files process_max_mono writes: io_ops.write_file(path, ..., suffix="max" / "min") -- no underscore"""
    stem = os.path.splitext(path)[0]
    return tuple(f"{stem}{s}.wav" for s in SUFFIXES)


def process(path, fft_size=FFT_SIZE, overlap=OVERLAP, device=None, signal_data=None):
    """The GUI's flow on one file: read `path` (signal_data=(signal, sr, channels) skips the read), MaxMono at hop =
    fft_size // overlap, write <stem>max.wav and <stem>min.wav (mono float32 WAV).  Returns the two paths.  A file that is not
    stereo raises ValueError."""
    signal, sr, num_channels = io_ops.read_file(path) if signal_data is None else signal_data
    if num_channels != 2 or signal.ndim != 2:
        raise ValueError(f"{path}: expects stereo input, got {num_channels} channel(s)")
    hop = int(fft_size) // int(overlap)
    y_max, y_min = max_mono(signal, sr, fft_size, hop, device=device)
    for y, suffix in zip((y_max, y_min), SUFFIXES):
        io_ops.write_file(path, y, sr, 1, suffix=suffix)
    return output_paths(path)
