"""Mirror of reference util/decompose.py -- hpss, harmonic, softmask, magphase with the same names, argument order and defaults;
the two median filters, the soft masks and the products run in one HIP kernel (par_hpss_f32, csrc/hpss.hip).

    H, P = hpss(S)                                  # S: (bins, frames), numpy (any memory order) or a device tensor
    mask_h, mask_p = hpss(S, mask=True)
    H = harmonic(S, kernel_size=(31, 17), margin=(1.0, 3.0))

numpy in, numpy out; a device tensor in (the (bins, frames) view of a frame-major buffer that fourier.stft / stft_dev return)
gives device tensors of the same layout, ready for fourier.istft.  Per bin: harm = median of |S| over kernel_size[0] frames,
perc = median of |S| over kernel_size[1] bins (scipy.ndimage.median_filter, mode "reflect": rank k // 2, kernels 1..99, odd or
even), mask_h = softmask(harm, perc * margin_h), mask_p = softmask(perc, harm * margin_p), H = S * mask_h, P = S * mask_p.

Differences from the reference:
- float64 / complex128 input is computed in float32 / complex64 and returned so (the reference's torch and pyfftw STFT
  backends yield complex64; its numpy backend's division by sqrt(n_fft) promotes to complex128 under numpy 2).
- H and P are S * mask; the reference multiplies (|S| * mask) by exp(i angle(S)), which is the same number up to rounding.
- Where the reference prints a message and returns None (softmask: shape mismatch, negative input, power <= 0) or hits a
  NameError (hpss: a margin below 1), ValueError is raised; harmonic's margin check raises too (the reference only prints).
- harmonic takes |S| of a complex S like hpss does (the reference hands the complex array to median_filter).
- Kernel sizes outside 1..99 raise ValueError (the GUI offers 1..99).
- softmask and magphase are small host functions on numpy arrays (float32 for integer input), not device entry points; the
  kernel states the same mask rule in float32 (csrc/hpss.hip).
- A real numpy spectrogram with negative values raises ValueError; the kernel itself takes fabs of real input, so -0.0 counts
  as 0 and a real device tensor is read by magnitude.
"""
import numpy as np
import torch

from . import _dev, _lib

MAX_KERNEL = 99          # PAR_HPSS_MAX_KERNEL


def softmask(X, X_ref, power=1, split_zeros=False):
    """Share of X in X and X_ref after raising both to `power`, between 0 and 1 per element.  Both are first divided by the
    larger of the pair, which leaves the share as it is and keeps the powers in range.  Where even the larger one is under the
    smallest normal number of the result type there is nothing to share out: such elements get 0.5 (split_zeros) or 0.  An
    infinite power gives the boolean mask X > X_ref.  Host arrays; integers are computed in float32."""
    if not power > 0:
        raise ValueError(f"softmask: power has to be above zero (got {power})")
    x, ref = np.asarray(X), np.asarray(X_ref)
    if x.shape != ref.shape:
        raise ValueError(f"softmask: X has shape {x.shape}, X_ref has shape {ref.shape}")
    for name, v in (("X", x), ("X_ref", ref)):
        if v.size and v.min() < 0:
            raise ValueError(f"softmask: {name} holds negative values; magnitudes are expected")
    if np.isinf(power):
        return np.greater(x, ref)
    ftype = x.dtype if np.issubdtype(x.dtype, np.floating) else np.dtype(np.float32)
    larger = np.maximum(x, ref).astype(ftype)
    empty = larger < np.finfo(ftype).tiny
    scale = np.where(empty, ftype.type(1), larger)
    with np.errstate(invalid="ignore", divide="ignore"):
        own, other = np.power(x / scale, power), np.power(ref / scale, power)
        share = own / (own + other)
    return np.where(empty, ftype.type(0.5 if split_zeros else 0.0), share).astype(ftype, copy=False)


def magphase(D, power=1):
    """(magnitude, phase) of a spectrogram with D = |D| * phase: magnitude is |D| ** power, phase the unit complex number
    along D (1 where D is zero), built from cos and sin of D's angle.  Host arrays."""
    D = np.asarray(D)
    angle = np.arctan2(D.imag, D.real)
    phase = (np.cos(angle) + 1j * np.sin(angle)).astype(np.result_type(D.dtype, np.complex64), copy=False)
    return np.power(np.abs(D), power), phase


def _pair(v):
    if np.isscalar(v):
        return v, v
    return v[0], v[1]


def _check(kernel_size, power, margin):
    win_harm, win_perc = _pair(kernel_size)
    margin_harm, margin_perc = _pair(margin)
    for k in (win_harm, win_perc):
        if int(k) != k or not 1 <= k <= MAX_KERNEL:
            raise ValueError(f"kernel sizes must be integers in 1..{MAX_KERNEL} (got {kernel_size})")
    if not power > 0:
        raise ValueError(f"power has to be above zero (got {power})")
    if margin_harm < 1 or margin_perc < 1:
        raise ValueError(f"a margin below 1 would let a component exceed the input (got {margin})")
    return int(win_harm), int(win_perc), float(power), float(margin_harm), float(margin_perc)


def hpss_dev(fm, win_harm, win_perc, power, margin_harm, margin_perc, out_kind=_lib.HPSS_COMPONENTS, dev=None, out=None):
    """par_hpss_f32 on a frame-major device spectrogram fm (frames, bins) (complex64 or float32; rows may be pitched: stride(0)
    >= bins, stride(1) == 1).  Returns (out_h, out_p) device tensors (frames, bins) of the same pitch -- the input's type for
    components, float32 for masks and medians; out_p is None for HPSS_HARMONIC.  out: an (out_h, out_p) pair to reuse."""
    dev = _dev.device_index(dev if dev is not None else fm.device)
    if fm.ndim != 2:
        raise ValueError(f"a spectrogram has two dimensions (got {tuple(fm.shape)})")
    if fm.dtype not in (torch.complex64, torch.float32):
        fm = fm.to(torch.complex64 if fm.is_complex() else torch.float32)
    if fm.shape[1] > 1 and fm.stride(1) != 1 or fm.shape[0] > 1 and fm.stride(0) < fm.shape[1]:
        fm = fm.contiguous()
    frames, bins = fm.shape
    if frames == 0 or bins == 0:
        raise ValueError(f"empty spectrogram {tuple(fm.shape)}")
    pitch = fm.stride(0) if frames > 1 else bins
    out_dtype = fm.dtype if out_kind in (_lib.HPSS_COMPONENTS, _lib.HPSS_HARMONIC) else torch.float32
    n_out = 1 if out_kind == _lib.HPSS_HARMONIC else 2
    if out is None:
        out = [_dev.empty((frames, pitch), out_dtype, dev) for _ in range(n_out)]
    for o in out[:n_out]:
        if o.shape != (frames, pitch) or o.dtype != out_dtype or not o.is_contiguous():
            raise ValueError("hpss_dev: output buffers must be contiguous (frames, pitch) tensors of the output type")
    _lib.check(_lib.lib().par_hpss_f32(dev, _dev.ptr(fm), int(fm.is_complex()), frames, bins, pitch, win_harm, win_perc, power, margin_harm,
                                       margin_perc, _dev.ptr(out[0]), _dev.ptr(out[1]) if n_out == 2 else None, out_kind,
                                       _dev.stream_ptr(dev)))
    return out[0][:, :bins], (out[1][:, :bins] if n_out == 2 else None)


def _run(S, kernel_size, power, margin, out_kind):
    win_harm, win_perc, power, margin_harm, margin_perc = _check(kernel_size, power, margin)
    if isinstance(S, torch.Tensor):
        if S.ndim != 2:
            raise ValueError(f"S must be (bins, frames) (got {tuple(S.shape)})")
        h, p = hpss_dev(S.T, win_harm, win_perc, power, margin_harm, margin_perc, out_kind)
        return h.T, (None if p is None else p.T)
    S = np.asarray(S)
    if S.ndim != 2:
        raise ValueError(f"S must be (bins, frames) (got {S.shape})")
    is_complex = np.iscomplexobj(S)
    if not is_complex and S.size and np.any(S < 0):
        raise ValueError("a real spectrogram must be non-negative (magnitudes)")
    dev = _dev.device_index(None)
    fm = _dev.to_dev(S.T, torch.complex64 if is_complex else torch.float32, dev)
    h, p = hpss_dev(fm, win_harm, win_perc, power, margin_harm, margin_perc, out_kind, dev)
    return _dev.to_host(h).T, (None if p is None else _dev.to_host(p).T)


def hpss(S, kernel_size=31, power=2.0, mask=False, margin=1.0):
    """Median-filtering harmonic / percussive separation: (H, P) with S = H + P for margin 1, S = H + P + R above it;
    (mask_H, mask_P) for mask=True (boolean arrays for power = inf, like the reference's)."""
    h, p = _run(S, kernel_size, power, margin, _lib.HPSS_MASKS if mask else _lib.HPSS_COMPONENTS)
    if mask and not np.isfinite(power):
        return h != 0, p != 0
    return h, p


def harmonic(S, kernel_size=31, power=2.0, mask=False, margin=1.0):
    """The harmonic component S * mask_H alone (`mask` is accepted and ignored, as in the reference)."""
    return _run(S, kernel_size, power, margin, _lib.HPSS_HARMONIC)[0]


def medians(S, kernel_size=31):
    """(harm, perc): the two median-filtered magnitude spectrograms hpss builds its masks from, float32."""
    return _run(S, kernel_size, 2.0, 1.0, _lib.HPSS_MEDIANS)
