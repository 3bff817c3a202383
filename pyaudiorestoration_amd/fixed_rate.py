"""Resampling by one constant ratio -- what the reference gets from
``resampy.resample(x, sr_orig, sr_new, axis=0, filter='sinc_window', num_zeros=8)`` at four call sites
(renoiser_gui.py:246, pytapesynch_gui.py:117-122, humspeed_gui.py:197 and experiments): Smith's band-limited interpolation over
resampy 0.4's interpolated filter table, in K_rsfix (par_resample_fixed_f32).  `resample` takes resampy's call shape, so a call
site changes one word.

This is not K_sinc (resampling.py): that is the reference's own time-varying windowed sinc with another window, cutoff and tap
rule.  Positions, table offsets and interpolation fractions are float64 on the device and equal numpy's bit for bit; the weights
and sums are float32 (resampy computes in the input's dtype, float64 sums for float64 input)."""
import numpy as np
import torch

from . import _dev, _lib

NUM_ZEROS = 8


def out_len(n, sr_orig, sr_new):
    """Samples written for n input samples: int(n * sr_new / sr_orig), as resampy sizes its output."""
    return int(_lib.lib().par_resample_fixed_out_len(int(n), float(sr_orig), float(sr_new)))


def resample_dev(x_t, n, ch, sr_orig, sr_new, num_zeros=NUM_ZEROS, out=None, dev=None):
    """Device-level form: x_t float32 device tensor holding (n, ch) interleaved samples (contiguous, any shape with n * ch
    elements) -> float32 device tensor (n_out, ch).  One launch per channel on strided views.  out: a contiguous float32
    (n_out, ch) tensor to fill."""
    dev = _dev.device_index(dev if dev is not None else x_t.device)
    L = _lib.lib()
    if x_t.dtype != torch.float32 or not x_t.is_contiguous() or x_t.numel() != n * ch:
        raise ValueError("resample_dev: x_t must be a contiguous float32 tensor of n * ch elements")
    sr_orig, sr_new = float(sr_orig), float(sr_new)
    n_out = int(L.par_resample_fixed_out_len(n, sr_orig, sr_new))
    if n_out < 0:
        raise ValueError(f"sample rates must be finite and positive (got {sr_orig} -> {sr_new})")
    if out is None:
        out = _dev.empty((n_out, ch), torch.float32, dev)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (n_out, ch):
        raise ValueError(f"resample_dev: out must be a contiguous float32 tensor of shape {(n_out, ch)}")
    stream = _dev.stream_ptr(dev)
    x_flat, y_flat = x_t.reshape(-1), out.reshape(-1)
    if n == 0 or n_out == 0:
        return out
    for c in range(ch):
        _lib.check(L.par_resample_fixed_f32(dev, _dev.ptr(x_flat[c:]), n, ch, sr_orig, sr_new, int(num_zeros), _dev.ptr(y_flat[c:]),
                                            n_out, ch, stream))
    return out


def resample(x, sr_orig, sr_new, axis=0, filter='sinc_window', num_zeros=NUM_ZEROS, device=None):
    """resampy.resample's call shape.  x: numpy array or device tensor, 1-D or (n, ch), time on axis 0 -> float32 of the same
    kind with int(n * sr_new / sr_orig) samples.  Only axis=0 and filter='sinc_window' (the reference's call) are supported."""
    if axis != 0:
        raise ValueError(f"fixed_rate.resample: only axis=0 is supported (got {axis})")
    if filter != 'sinc_window':
        raise ValueError(f"fixed_rate.resample: only filter='sinc_window' is supported (got {filter!r})")
    if not 1 <= int(num_zeros) <= 64:
        raise ValueError(f"fixed_rate.resample: num_zeros {num_zeros} outside 1..64")
    if x.ndim not in (1, 2):
        raise ValueError("fixed_rate.resample: x must be 1-D or (n, channels)")
    if not (np.isfinite(sr_orig) and np.isfinite(sr_new) and sr_orig > 0 and sr_new > 0):
        raise ValueError(f"sample rates must be finite and positive (got {sr_orig} -> {sr_new})")
    was_tensor = torch.is_tensor(x)
    dev = _dev.device_index(device if device is not None else (x.device if was_tensor and x.is_cuda else None))
    x2d = x if x.ndim == 2 else x[:, None]
    n, ch = x2d.shape
    x_t = _dev.to_dev(x2d, torch.float32, dev)
    out = resample_dev(x_t, n, ch, sr_orig, sr_new, num_zeros, dev=dev)
    res = out if x.ndim == 2 else out[:, 0]
    return res if was_tensor else _dev.to_host(res)
