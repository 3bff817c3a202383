"""The dynamics matcher of the reference's experiments/decompressor_cmd.py on the GPU: two same-length transfers of one recording,
the one to restore (src) and one with the intended dynamics (ref); src's dynamics are restored to those of ref.

    out = match_dynamics(src, ref, sr)                   # process (decompressor_cmd.py:26-188) without the files
    process("remaster.flac", "original.flac")            # ... and with them: writes remaster.flacdecompressed.wav

Chain (constants decompressor_cmd.py:41-55): zero-phase band-pass 80-9000 Hz of every channel of both files (one batched
K_sosfiltfilt call), windowed RMS at hop 32 / window 512 -> clip at 0.0005 -> log10 (par_windowed_rms_log10_f64), level match
(par_level_match_f64), box smoothing in scipy's default "reflect" mode (par_uniform_filter_reflect_f64), Hann overlap-add and
clipped gain (par_dynamics_factor_f64), np.interp onto the samples, channel mean and product (par_dynamics_apply_f32).

The reference's Hann overlap-add is kept as it is (do_sync is a constant False there): the window sum multiplies a LOG value,
and the last corr_hop .. 2 corr_hop frames of every file (up to 3 s at the defaults) carry half a window or none, so their
gain is min(10^b, 2).  The do_sync=True branch is dead code in the reference and is not ported."""
import logging

import numpy as np
import torch

from . import _dev, _lib, filters, io_ops

RMS_FLOOR = 0.0005              # decompressor_cmd.py:93-94
ORDER = 3                       # :86-87
_hann = {}


def _as_2d(signal):
    return signal if signal.ndim == 2 else signal[:, None]


def n_frames(n, hop):
    """len(range(0, n, hop)) (decompressor_cmd.py:18)"""
    return -(-int(n) // int(hop))


def smoothing_size(sr, smoothing_sec, hop):
    """The box filter's size in frames (decompressor_cmd.py:80); scipy raises for a size below 1."""
    ns = int(sr * smoothing_sec / hop)
    if ns < 1:
        raise ValueError(f"smoothing of {smoothing_sec} s at {sr} Hz and hop {hop} is {ns} frames: the filter size must be at least 1")
    return ns


def _hann_dev(corr_sz, dev):
    """np.hanning(corr_sz) (decompressor_cmd.py:79) in HBM: computed by numpy, uploaded once per (device, size)"""
    key = (dev, int(corr_sz))
    if key not in _hann:
        _hann[key] = _dev.to_dev(np.hanning(int(corr_sz)), torch.float64, dev)
    return _hann[key]


def windowed_rms_dev(rows_t, hop, sz, floor=0.0, log10=False, dev=None, out=None):
    """Windowed RMS of every row of a (rows, n) float64 device tensor -> (rows, ceil(n / hop)) float64; np.clip(., floor, None) and,
    with log10, its logarithm (par_windowed_rms_log10_f64)."""
    dev = _dev.device_index(dev if dev is not None else rows_t.device)
    if rows_t.ndim != 2 or rows_t.dtype != torch.float64 or rows_t.stride(1) != 1:
        raise ValueError("rows must be a (rows, n) float64 tensor with contiguous rows")
    rows, n = rows_t.shape
    if out is None:
        out = _dev.empty((rows, n_frames(n, hop)), torch.float64, dev)
    _lib.check(_lib.lib().par_windowed_rms_log10_f64(dev, _dev.ptr(rows_t), rows_t.stride(0) if rows > 1 else n, rows, n, int(hop), int(sz),
                                                     float(floor), int(bool(log10)), _dev.ptr(out), _dev.stream_ptr(dev)))
    return out


def windowed_rms(signal, hop, sz):
    """decompressor_cmd.windowed_rms (:16-23): the RMS of signal[i : i + sz] for i = 0, hop, 2 hop, .. < len(signal), the last
    windows truncated.  1-D numpy array or device tensor in, float64 of the same kind out."""
    was_tensor = torch.is_tensor(signal)
    dev = _dev.device_index(signal.device if was_tensor else None)
    x = _dev.to_dev(signal, torch.float64, dev)
    if x.ndim != 1:
        raise ValueError("signal must be one-dimensional")
    if x.numel() == 0:
        return x if was_tensor else np.zeros(0)
    out = windowed_rms_dev(x[None, :], hop, sz, 0.0, False, dev)[0]
    return out if was_tensor else _dev.to_host(out)


def gain_curves_dev(src_t, ref_t, sr, hop=32, sz=512, corr_sz=4096, smoothing_sec=0.08, lower=80, upper=9000, dev=None,
                    aligned_out=None):
    """(n, ch) float32 device tensors of equal shape -> fac (ch, F) float64 device tensor, F = ceil(n / hop): steps
    decompressor_cmd.py:83-166 for every channel.  aligned_out: a (ch, F) float64 tensor that receives the overlap-added curve."""
    dev = _dev.device_index(dev if dev is not None else src_t.device)
    if src_t.shape != ref_t.shape or src_t.ndim != 2:
        raise ValueError(f"src and ref must be (n, ch) arrays of one shape, got {tuple(src_t.shape)} and {tuple(ref_t.shape)}")
    ns = smoothing_size(sr, smoothing_sec, hop)
    n, ch = src_t.shape
    L, stream = _lib.lib(), _dev.stream_ptr(dev)
    rows = _dev.empty((2 * ch, n), torch.float64, dev)                 # src channels, then ref channels
    rows[:ch].copy_(src_t.T)
    rows[ch:].copy_(ref_t.T)
    band = filters.bandpass_batch_dev(rows, lower, upper, sr, order=ORDER, dev=dev)
    F = n_frames(n, hop)
    curves = windowed_rms_dev(band, hop, sz, RMS_FLOOR, True, dev)
    del band, rows
    matched = _dev.empty((2 * ch, F), torch.float64, dev)              # a as it is, b level-matched: one smoothing call for both
    matched[:ch].copy_(curves[:ch])
    _lib.check(L.par_level_match_f64(dev, _dev.ptr(curves[:ch]), _dev.ptr(curves[ch:]), ch, F, _dev.ptr(matched[ch:]), stream))
    smooth = curves                                                    # reused: the raw curves are no longer needed
    _lib.check(L.par_uniform_filter_reflect_f64(dev, _dev.ptr(matched), 2 * ch, F, ns, _dev.ptr(smooth), stream))
    fac = _dev.empty((ch, F), torch.float64, dev)
    _lib.check(L.par_dynamics_factor_f64(dev, _dev.ptr(smooth[:ch]), _dev.ptr(smooth[ch:]), ch, F, _dev.ptr(_hann_dev(corr_sz, dev)),
                                         int(corr_sz), None if aligned_out is None else _dev.ptr(aligned_out), _dev.ptr(fac), stream))
    return fac


def gain_curves(src, ref, sr, hop=32, sz=512, corr_sz=4096, smoothing_sec=0.08, lower=80, upper=9000):
    """fac (ch, F) of decompressor_cmd.py:161-166 for two (n, ch) (or (n,)) float32 signals of one shape; numpy in, numpy out, device
    tensors in, device tensor out."""
    was_tensor = torch.is_tensor(src)
    smoothing_size(sr, smoothing_sec, hop)
    if _as_2d(src).shape != _as_2d(ref).shape:
        raise ValueError(f"src and ref must be arrays of one shape, got {tuple(src.shape)} and {tuple(ref.shape)}")
    dev = _dev.device_index(src.device if was_tensor else None)
    fac = gain_curves_dev(_dev.to_dev(_as_2d(src), torch.float32, dev), _dev.to_dev(_as_2d(ref), torch.float32, dev), sr, hop, sz, corr_sz,
                          smoothing_sec, lower, upper, dev)
    return fac if was_tensor else _dev.to_host(fac)


def apply_gain_dev(src_t, fac, hop, dev=None):
    """(n, ch) float32 device tensor and fac (ch, F) -> float32(src * mean over channels of np.interp(i, j hop, fac[c]))"""
    dev = _dev.device_index(dev if dev is not None else src_t.device)
    n, ch = src_t.shape
    out = _dev.empty((n, ch), torch.float32, dev)
    _lib.check(_lib.lib().par_dynamics_apply_f32(dev, _dev.ptr(src_t), ch, ch, n, _dev.ptr(fac), fac.shape[1], int(hop), _dev.ptr(out), ch,
                                                 _dev.stream_ptr(dev)))
    return out


def match_dynamics_dev(src_t, ref_t, sr, hop=32, sz=512, corr_sz=4096, smoothing_sec=0.08, lower=80, upper=9000, dev=None):
    """match_dynamics on (n, ch) float32 device tensors of one shape; the result stays in HBM."""
    dev = _dev.device_index(dev if dev is not None else src_t.device)
    src_t = src_t.contiguous()
    fac = gain_curves_dev(src_t, ref_t, sr, hop, sz, corr_sz, smoothing_sec, lower, upper, dev)
    return apply_gain_dev(src_t, fac, hop, dev)


def match_dynamics(src, ref, sr, hop=32, sz=512, corr_sz=4096, smoothing_sec=0.08, lower=80, upper=9000, device=None):
    """decompressor_cmd.process on two (n, ch) (or (n,)) float32 signals: src with the dynamics of ref, float32 (n, ch).  numpy in,
    numpy out; device tensors in, device tensor out.  Unequal lengths are truncated to the shorter (with a log line, like the
    reference's print); unequal channel counts raise ValueError."""
    was_tensor = torch.is_tensor(src)
    src2, ref2 = _as_2d(src), _as_2d(ref)
    if src2.shape[1] != ref2.shape[1]:
        raise ValueError("Both files must have the same amount of channels!")
    smoothing_size(sr, smoothing_sec, hop)
    dev = _dev.device_index(device if device is not None else (src.device if was_tensor else None))
    if len(src2) != len(ref2):
        logging.warning("Both files must have the same amount of samples! Truncated %s", "source to ref" if len(ref2) < len(src2) else "ref to source")
        m = min(len(src2), len(ref2))
        src2, ref2 = src2[:m], ref2[:m]
    out = match_dynamics_dev(_dev.to_dev(src2, torch.float32, dev), _dev.to_dev(ref2, torch.float32, dev), sr, hop, sz, corr_sz,
                             smoothing_sec, lower, upper, dev)
    return out if was_tensor else _dev.to_host(out)


def process(filename_src, filename_ref, device=None):
    """decompressor_cmd.process: reads both files (io_ops.read_file), matches, writes filename_src + 'decompressed.wav' as float32
    WAV (the reference's name and subtype) and returns that path.  Differing sample rates or channel counts raise ValueError
    (the reference prints and returns)."""
    src, sr, ch = io_ops.read_file(filename_src)
    ref, sr_ref, ch_ref = io_ops.read_file(filename_ref)
    if sr != sr_ref:
        raise ValueError("Both files must have the same sample rate!")
    if ch != ch_ref:
        raise ValueError("Both files must have the same amount of channels!")
    out = match_dynamics(src, ref, sr, device=device)
    path = filename_src + "decompressed.wav"
    io_ops.write_wav_float(path, out, sr)
    return path
