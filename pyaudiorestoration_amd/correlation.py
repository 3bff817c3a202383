"""Correlation helpers with the call contracts of the reference's util/correlation.py (xcorr :6-13,
find_delay :16-39, parabolic :42-46), on the device: `par_xcorr_f64` / `par_find_delay_f64` (csrc/stft.hip) run the
correlation through one complex four-step FFT of a/|a| + i b/|b|; find_delay re-evaluates the lags around the peak as
float64 dot products before the parabolic refinement, so the delay the tape-sync tool reads is exact.  The delay search
is written once: `par_find_delay_batch_f64` decides W pairs of rows on the device, `par_find_delay_f64` is its W = 1
through the same kernels and waits once, for delay, corr and the row's status (the reference's IndexError).
"""
import ctypes
import logging

import numpy as np
import torch
from scipy.signal import get_window

from . import _dev, _lib


def _centre(full, n, m, mode):
    if mode == "full":
        return full
    if mode == "same":                       # size of the first input, centred on the 'full' output (scipy)
        start = (m - 1) // 2
        return full[..., start:start + n]
    if mode == "valid":
        lo, hi = min(n, m), max(n, m)
        return full[..., lo - 1:hi]
    raise ValueError(f"unknown correlation mode {mode!r}")


def _up(a, dev):
    return a.to(device=f"cuda:{dev}", dtype=torch.float64) if isinstance(a, torch.Tensor) else \
        _dev.to_dev(a, torch.float64, dev)                  # float32 signals cross PCIe as they are and widen in HBM


def xcorr_dev(a_t, b_t, dev=None):
    """'full' normalised cross-correlation of two 1-D float64 device tensors -> float64 device tensor."""
    dev = _dev.device_index(dev if dev is not None else a_t.device)
    L = _lib.lib()
    na, nb = a_t.numel(), b_t.numel()
    nbytes = int(L.par_xcorr_scratch_bytes(na, nb))
    scratch = _dev.empty(max(nbytes, 1), torch.uint8, dev)
    full = _dev.empty(na + nb - 1, torch.float64, dev)
    _lib.check(L.par_xcorr_f64(dev, _dev.ptr(a_t), na, _dev.ptr(b_t), nb, _dev.ptr(scratch), nbytes, _dev.ptr(full),
                               _dev.stream_ptr(dev)))
    return full


def xcorr(a, b, mode='full'):
    """Normalised cross-correlation in [-1, 1] of two 1-D signals (scipy.signal.correlate conventions)."""
    dev = _dev.device_index(None)
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 1 or b.ndim != 1 or len(a) < 1 or len(b) < 1:
        raise ValueError("xcorr needs two non-empty 1-D signals")
    full = xcorr_dev(_up(a, dev), _up(b, dev), dev).cpu().numpy()
    return _centre(full, len(a), len(b), mode)


def parabolic(f, x):
    """Vertex (position, height) of the parabola through f[x-1], f[x], f[x+1]."""
    left, mid, right = f[x - 1], f[x], f[x + 1]
    slope2 = left - right                                  # twice the centred difference
    xv = x + 0.5 * slope2 / (left - 2 * mid + right)
    return xv, mid - 0.25 * slope2 * (xv - x)


def find_delay(a, b, ignore_phase=False, window_name=None):
    """Delay in samples (fractional) between 1-D signals a and b, and the correlation there.
    Like the reference, a given window is applied to `a` and `b` IN PLACE."""
    for sig in ((a, b) if window_name else ()):
        if isinstance(sig, torch.Tensor):          # device-resident signals (pipeline.correlate_sources): windowed in HBM
            sig.mul_(torch.from_numpy(get_window(window_name, sig.numel())).to(device=sig.device, dtype=sig.dtype))
        else:
            sig *= get_window(window_name, len(sig))
    if ignore_phase:
        logging.warning("Ignoring phase")
    dev = _dev.device_index(None)
    L = _lib.lib()
    a_t, b_t = _up(a, dev), _up(b, dev)
    na, nb = a_t.numel(), b_t.numel()
    nbytes = int(L.par_xcorr_scratch_bytes(na, nb))
    scratch = _dev.empty(max(nbytes, 1), torch.uint8, dev)
    delay, corr = ctypes.c_double(0.0), ctypes.c_double(0.0)
    _lib.check(L.par_find_delay_f64(dev, _dev.ptr(a_t), na, _dev.ptr(b_t), nb, int(bool(ignore_phase)), _dev.ptr(scratch), nbytes,
                                    ctypes.byref(delay), ctypes.byref(corr), _dev.stream_ptr(dev)))
    logging.debug(f"i_peak {delay.value + na // 2}")
    return delay.value, corr.value


def batch_scratch_bytes(na, nb, n_win):
    """Device bytes par_find_delay_batch_f64 asks for to take all windows in one pass; raises ParUnsupported for a shape
    the batch does not take (na + nb - 1 > 2^20: the sectioned form)."""
    L = _lib.lib()
    nbytes = int(L.par_find_delay_batch_scratch_bytes(na, nb, n_win))
    if nbytes == 0:
        raise _lib.ParUnsupported(3, f"find_delay_batch: windows of {na} and {nb} samples need the sectioned form (or are empty)")
    return nbytes


def find_delay_batch_dev(a_t, b_t, ignore_phase=False, window_name=None, dev=None, scratch_bytes=None):
    """find_delay for every pair of rows of two 2-D float64 device tensors (W, na) and (W, nb) (row stride >= row length,
    unit element stride) in one call: -> (delays, corrs, status) device tensors of length W, status 1 where the peak sits
    on the last lag (the reference's IndexError; that row's delay and corr are NaN).  A given window is applied to the
    rows IN PLACE, like find_delay.  Raises nothing for a row's status; scratch_bytes: device bytes for the passes
    (default: what the library asks for)."""
    dev = _dev.device_index(dev if dev is not None else a_t.device)
    if a_t.ndim != 2 or b_t.ndim != 2 or a_t.shape[0] != b_t.shape[0]:
        raise ValueError("find_delay_batch needs (W, na) and (W, nb)")
    W, na = a_t.shape
    nb = b_t.shape[1]
    if a_t.dtype != torch.float64 or b_t.dtype != torch.float64 or (W and (a_t.stride(1) != 1 or b_t.stride(1) != 1)):
        raise ValueError("find_delay_batch_dev needs float64 rows of unit element stride")
    L = _lib.lib()
    delays = _dev.empty(W, torch.float64, dev)
    corrs = _dev.empty(W, torch.float64, dev)
    status = _dev.empty(W, torch.int32, dev)
    if W == 0:
        return delays, corrs, status
    nbytes = batch_scratch_bytes(na, nb, W) if scratch_bytes is None else int(scratch_bytes)
    scratch = _dev.empty(max(nbytes, 1), torch.uint8, dev)
    win_a = win_b = None
    if window_name:
        win_a = _dev.to_dev(get_window(window_name, na), torch.float64, dev)
        win_b = _dev.to_dev(get_window(window_name, nb), torch.float64, dev)
    _lib.check(L.par_find_delay_batch_f64(dev, _dev.ptr(a_t), a_t.stride(0) if W > 1 else max(a_t.stride(0), na), na, _dev.ptr(b_t),
                                          b_t.stride(0) if W > 1 else max(b_t.stride(0), nb), nb, W,
                                          _dev.ptr(win_a) if window_name else None, _dev.ptr(win_b) if window_name else None,
                                          int(bool(ignore_phase)), _dev.ptr(scratch), nbytes, _dev.ptr(delays), _dev.ptr(corrs),
                                          _dev.ptr(status), _dev.stream_ptr(dev)))
    return delays, corrs, status


def find_delay_batch(a, b, ignore_phase=False, window_name=None):
    """find_delay(a[w], b[w]) for every row w of a (W, na) and b (W, nb), numpy or float64 device tensors -> (delays, corrs),
    float64 numpy arrays of length W.  Like find_delay, a given window is applied to `a` and `b` IN PLACE.  The first row
    whose peak sits on the last lag raises the reference's IndexError, with the row's index."""
    if ignore_phase:
        logging.warning("Ignoring phase")
    dev = _dev.device_index(None)
    a_t, b_t = (s if isinstance(s, torch.Tensor) else _dev.to_dev(np.asarray(s), torch.float64, dev) for s in (a, b))
    delays, corrs, status = find_delay_batch_dev(a_t, b_t, ignore_phase, window_name, dev)
    for host, t in ((a, a_t), (b, b_t)):
        if window_name and not isinstance(host, torch.Tensor):      # the in-place contract for host arrays
            host[...] = _dev.to_host(t)
    status = status.cpu().numpy()
    bad = np.flatnonzero(status == 1)
    if len(bad):
        na = a_t.shape[1]
        raise IndexError(f"index {na} is out of bounds for axis 0 with size {na} (row {int(bad[0])})")
    return _dev.to_host(delays), _dev.to_host(corrs)


MAX_ROW = 1 << 25                       # samples per row of find_delay_rows (par_find_delay_sect_f64)


def _auto_section(na, nb):
    """section_log2 for rows of na and nb samples: the smallest section that holds a whole row (one section pair, the
    smallest transforms) up to the library's default 2^19.  The results do not depend on the choice."""
    lg = 12
    while (1 << lg) < max(na, nb) and lg < 19:
        lg += 1
    return lg


def find_delay_rows_dev(a_t, b_t, ignore_phase=False, section=None, want_norms=False, want_same=False, scratch_bytes=None):
    """find_delay for every pair of rows of two 2-D float64 device tensors (W, na) and (W, nb) of ANY length up to 2^25
    (row stride >= row length, unit element stride), in one call and without a host wait: par_find_delay_sect_f64 cuts
    the rows into sections of 2^section samples (12..19, 0 = 19; None: the smallest that holds a row) and correlates them
    diagonal by diagonal.  The rows are only read.  -> (delays, corrs, status[, norms (W, 2)][, same (W, na)]) device
    tensors; status 1 where the peak sits on the last lag (that row's delay and corr are NaN).  scratch_bytes: device
    bytes for the passes (default: what the library asks for)."""
    dev = _dev.device_index(a_t.device)
    if a_t.ndim != 2 or b_t.ndim != 2 or a_t.shape[0] != b_t.shape[0]:
        raise ValueError("find_delay_rows needs (W, na) and (W, nb)")
    W, na = a_t.shape
    nb = b_t.shape[1]
    if a_t.dtype != torch.float64 or b_t.dtype != torch.float64 or (W and (a_t.stride(1) != 1 or b_t.stride(1) != 1)):
        raise ValueError("find_delay_rows_dev needs float64 rows of unit element stride")
    sec = _auto_section(na, nb) if section is None else int(section)
    L = _lib.lib()
    delays = _dev.empty(W, torch.float64, dev)
    corrs = _dev.empty(W, torch.float64, dev)
    status = _dev.empty(W, torch.int32, dev)
    norms = _dev.empty((W, 2), torch.float64, dev) if want_norms else None
    same = _dev.empty((W, na), torch.float64, dev) if want_same else None
    out = (delays, corrs, status) + ((norms,) if want_norms else ()) + ((same,) if want_same else ())
    if W:
        nbytes = int(L.par_find_delay_sect_scratch_bytes(na, nb, W, sec)) if scratch_bytes is None else int(scratch_bytes)
        scratch = _dev.empty(max(nbytes, 1), torch.uint8, dev)
        _lib.check(L.par_find_delay_sect_f64(dev, _dev.ptr(a_t), a_t.stride(0) if W > 1 else max(a_t.stride(0), na), na,
                                             _dev.ptr(b_t), b_t.stride(0) if W > 1 else max(b_t.stride(0), nb), nb, W, sec,
                                             int(bool(ignore_phase)), _dev.ptr(scratch), nbytes, _dev.ptr(delays), _dev.ptr(corrs),
                                             _dev.ptr(status), _dev.ptr(norms) if want_norms else None,
                                             _dev.ptr(same) if want_same else None, na, _dev.stream_ptr(dev)))
    return out


def find_delay_rows(a, b, ignore_phase=False, section=None, want_norms=False, want_same=False, scratch_bytes=None):
    """find_delay(a[w], b[w]) for every row w of a (W, na) and b (W, nb), numpy or float64 device tensors, rows of any
    length up to 2^25 -> (delays, corrs[, norms][, same]) as numpy arrays.  The first row whose peak sits on the last lag
    raises the reference's IndexError, with the row's index."""
    if ignore_phase:
        logging.warning("Ignoring phase")
    dev = _dev.device_index(None)
    a_t, b_t = (s if isinstance(s, torch.Tensor) else _dev.to_dev(np.asarray(s), torch.float64, dev) for s in (a, b))
    out = find_delay_rows_dev(a_t, b_t, ignore_phase, section, want_norms, want_same, scratch_bytes)
    bad = np.flatnonzero(out[2].cpu().numpy() == 1)
    if len(bad):
        na = a_t.shape[1]
        raise IndexError(f"index {na} is out of bounds for axis 0 with size {na} (row {int(bad[0])})")
    return tuple(_dev.to_host(t) for t in out[:2] + out[3:])
