"""numpy / scipy statement of median-filtering harmonic / percussive separation, for the tests (our own words for the rules of
decompose.hpss): harm and perc are scipy.ndimage.median_filter of the magnitudes along time and along frequency (mode
"reflect"), each mask compares one median with the other times its margin, relative to the larger of the two, in float32.

Everything takes and returns arrays of logical shape (bins, frames)."""
import numpy as np
import scipy.ndimage

TINY = np.finfo(np.float32).tiny


def reflect_indices(n, k):
    """source index of every tap of every output of a size-k "reflect" filter along an axis of length n: (n, k) ints; tap j of
    output i looks at position i - k // 2 + j, mirrored about the half samples at both ends as often as needed"""
    pos = np.arange(n)[:, None] - k // 2 + np.arange(k)[None, :]
    m = np.mod(pos, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def median_reflect(mag, k, axis):
    """the element of rank k // 2 of every window, from reflect_indices (an independent check of scipy's filter)"""
    mag = np.moveaxis(np.asarray(mag), axis, -1)
    idx = reflect_indices(mag.shape[-1], k)
    out = np.sort(mag[..., idx], axis=-1)[..., k // 2]
    return np.moveaxis(out, -1, axis)


def medians(mag, win_harm, win_perc):
    mag = np.asarray(mag, dtype=np.float32)
    harm = scipy.ndimage.median_filter(mag, size=(1, win_harm), mode="reflect")
    perc = scipy.ndimage.median_filter(mag, size=(win_perc, 1), mode="reflect")
    return harm, perc


def mask(x, xref, power, both_margins_one):
    """float32 soft mask of x against xref"""
    x, xref = np.asarray(x, np.float32), np.asarray(xref, np.float32)
    if np.isinf(power):
        return x > xref
    z = np.maximum(x, xref)
    small = z < TINY
    z = np.where(small, np.float32(1), z)
    with np.errstate(all="ignore"):
        a = (x / z) ** power
        b = (xref / z) ** power
        m = a / (a + b)
    assert m.dtype == np.float32
    return np.where(small, np.float32(0.5 if both_margins_one else 0.0), m)


def mask64(x, xref, power, both_margins_one):
    """the soft mask with its arithmetic in float64: the ratios x / z and xref / z are the float32 quotients both the kernel and
    `mask` form, the power, the sum and the quotient are float64, rounded to float32 once.  The exponent is the float32 value of
    `power`, which is what numpy raises a float32 array to and what the kernel passes to powf (0.3 is float32(0.3) on both sides;
    with the float64 0.3, 1e-30 ** 0.3 alone moves by 8 float32 ulp).  A NaN in x or xref passes through np.maximum into z and
    from there into the mask, as in `mask`."""
    x, xref = np.asarray(x, np.float32), np.asarray(xref, np.float32)
    if np.isinf(power):
        return x > xref
    z = np.maximum(x, xref)
    small = z < TINY
    z = np.where(small, np.float32(1), z)
    with np.errstate(all="ignore"):
        a, b = x / z, xref / z
        assert a.dtype == b.dtype == np.float32
        a, b = a.astype(np.float64) ** float(np.float32(power)), b.astype(np.float64) ** float(np.float32(power))
        m = (a / (a + b)).astype(np.float32)
    return np.where(small, np.float32(0.5 if both_margins_one else 0.0), m)


def ulp_distance_nan(a, b):
    """(the NaN patterns are the same, largest float32 ulp distance over the cells that are NaN in neither)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    ok = ~(na | nb)
    return bool(np.array_equal(na, nb)), ulp_distance(a[ok], b[ok])


def masks(mag, kernel=(31, 31), power=2.0, margin=(1.0, 1.0)):
    harm, perc = medians(mag, *kernel)
    one = margin[0] == 1 and margin[1] == 1
    return mask(harm, perc * margin[0], power, one), mask(perc, harm * margin[1], power, one)


def hpss(spec, kernel=(31, 31), power=2.0, margin=(1.0, 1.0)):
    """(H, P) = spec * mask_h, spec * mask_p"""
    spec = np.asarray(spec)
    mh, mp = masks(np.abs(spec), kernel, power, margin)
    return spec * mh.astype(np.float32), spec * mp.astype(np.float32)


def hpss_polar(spec, kernel=(31, 31), power=2.0, margin=(1.0, 1.0)):
    """(H, P) in the order of operations of decompose.hpss: (|spec| * mask) * exp(i angle(spec)).  The unit phasor is rebuilt
    from a float32 angle, so this differs from spec * mask by a few units in the last place of the modulus."""
    spec = np.asarray(spec)
    mag = np.abs(spec)
    phase = np.exp(1j * np.angle(spec))
    mh, mp = masks(mag, kernel, power, margin)
    return (mag * mh) * phase, (mag * mp) * phase


def ulp_distance(a, b):
    """largest distance in float32 units in the last place between two float32 arrays of one sign pattern (complex: per part)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if np.iscomplexobj(a):
        a, b = a.astype(np.complex64).view(np.float32), b.astype(np.complex64).view(np.float32)
    ia = a.astype(np.float32).view(np.int32).astype(np.int64)
    ib = b.astype(np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int(np.max(np.abs(ia - ib))) if ia.size else 0
