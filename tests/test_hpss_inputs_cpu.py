"""Preconditions of tests/test_hpss_kernels_gpu.py, checked without a GPU: the oracle `hpss_np.median_reflect` against scipy and
against windows cut from np.pad(mode="symmetric"), that every value class of tests/hpss_inputs.py holds what its name says, that
the mask pair table puts every listed (harm, perc) pair where the GPU test expects it, numpy's own values on the complex special
cells, and the distance E_np of numpy's float32 mask from the float64 statement (printed, pytest -s, for NOTES.md)."""
import numpy as np
import pytest
import scipy.ndimage

import hpss_inputs as I
import hpss_np

NAN_FREE = ("uniform", "ties", "lowbit", "wide")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cells(z):
    return np.ascontiguousarray(z).view(np.uint64)


def windows(mag, k, axis):
    """(..., n, k): the reflected windows of median_reflect, cut from numpy's symmetric padding"""
    mag = np.moveaxis(np.asarray(mag), axis, -1)
    pad = [(0, 0)] * (mag.ndim - 1) + [(k // 2, k - 1 - k // 2)]
    p = np.pad(mag, pad, mode="symmetric")
    return np.stack([p[..., i:i + k] for i in range(mag.shape[-1])], axis=-2)


def test_axis_lengths_and_kernel_pairs_are_the_ones_the_kernel_branches_on():
    assert I.AXIS_LENGTHS == (1, 2, 3, 4, 5, 12, 13, 63, 64, 65, 67, 127, 128, 129, 130)
    assert I.KERNEL_PAIRS == ((1, 1), (2, 3), (3, 2), (4, 5), (5, 4), (31, 17), (98, 99), (99, 98))
    last_tile = {n - 64 * ((n - 1) // 64) for n in I.AXIS_LENGTHS}         # cells in the last 64-wide tile
    assert {1, 2, 3, 4, 5, 12, 13, 63, 64} <= last_tile                    # runs of 4: whole, 1, 2 and 3 over; a full tile
    assert max(I.AXIS_LENGTHS) <= 130 and max(max(s) for s in I.CORNER_SHAPES + I.CLASS_SHAPES) <= 130
    assert any(k // 2 >= 4 * n for n in I.AXIS_LENGTHS for k, _ in I.KERNEL_PAIRS)    # lengths where scipy is not defined


@pytest.mark.parametrize("cls", NAN_FREE)
def test_median_reflect_equals_scipy_where_scipy_is_defined(cls):
    checked = 0
    for n in I.AXIS_LENGTHS:
        a = I.magnitudes(I.make(cls, (n, 7), 11 + n))
        for k in sorted({k for pair in I.KERNEL_PAIRS for k in pair}):
            if not k // 2 < 4 * n:                                          # NOTES.md, HPSS: scipy reads element -1 past that
                continue
            want = scipy.ndimage.median_filter(a, size=(k, 1), mode="reflect")
            assert np.array_equal(bits(hpss_np.median_reflect(a, k, 0)), bits(want)), (cls, n, k)
            want = scipy.ndimage.median_filter(a.T.copy(), size=(1, k), mode="reflect")
            assert np.array_equal(bits(hpss_np.median_reflect(a.T.copy(), k, 1)), bits(want)), (cls, n, k)
            checked += 1
    assert checked > 80


@pytest.mark.parametrize("cls", I.REAL_CLASSES)
def test_median_reflect_equals_symmetric_padding_at_every_length(cls):
    for n in I.AXIS_LENGTHS:
        a = I.magnitudes(I.make(cls, (n, 5), 21 + n))
        for k in sorted({k for pair in I.KERNEL_PAIRS for k in pair}):
            want = np.sort(windows(a, k, 0), axis=-1)[..., k // 2]          # (5, n)
            got = hpss_np.median_reflect(a, k, 0)
            assert np.array_equal(bits(got), bits(want.T)), (cls, n, k)


def test_uniform_has_no_ties_and_wide_spans_the_finite_range():
    for shape in I.CLASS_SHAPES:
        u = I.uniform(shape, 1)
        assert u.dtype == np.float32 and u.shape == shape and len(np.unique(u)) > 0.99 * u.size and (u >= 0).all()
        w = bits(I.wide(shape, 1))
        assert (w <= I.INF_BITS).all()
        for value in (0, 1, I.FLT_MIN_BITS - 1, I.FLT_MIN_BITS, I.FLT_MAX_BITS, I.INF_BITS):
            assert (w == value).any(), (shape, hex(value))
        assert ((w > 0) & (w < I.FLT_MIN_BITS)).mean() > 0.05 and (w == I.INF_BITS).mean() < 0.05
        exps = np.unique(w >> 23)
        assert len(exps) > 100 and exps.min() == 0 and exps.max() == 255
        s = I.signed(shape, 1)
        assert np.array_equal(bits(np.abs(s)), w) and np.signbit(s).mean() > 0.3 and (~np.signbit(s)).mean() > 0.3
        assert (bits(s) == 0x80000000).any() and (bits(s) == 0).any()       # -0.0 and +0.0
        assert np.array_equal(bits(I.magnitudes(s)), w)


def test_ties_and_lowbit_windows():
    """per window of 3 or more: `ties` repeats the selected value, `lowbit` differs in the two lowest bits only"""
    for shape in I.CLASS_SHAPES:
        t, lo = I.ties(shape, 2), I.lowbit(shape, 2)
        assert set(np.unique(bits(t))) == {0, I.ONE_BITS, I.ONE_BITS + 1}
        assert set(np.unique(bits(lo))) == {I.LOWBIT_BASE + i for i in range(4)} and I.LOWBIT_BASE & 3 == 0
        for axis in (0, 1):
            for k in (3, 5, 17):
                w = windows(t, k, axis)
                med = np.sort(w, axis=-1)[..., k // 2]
                repeats = (bits(w) == bits(med)[..., None]).sum(axis=-1)
                below = (w < med[..., None]).sum(axis=-1)
                assert (repeats >= 2).mean() > 0.7, (shape, axis, k)        # cnt == rank is not the only way to the answer:
                assert (below < k // 2).mean() > 0.3, (shape, axis, k)      # fewer than `rank` lie strictly below the median
                ulp_apart = ((bits(w) == I.ONE_BITS).any(axis=-1) & (bits(w) == I.ONE_BITS + 1).any(axis=-1))
                assert ulp_apart.mean() > 0.3
                w = bits(windows(lo, k, axis))
                assert ((w >> 2) == I.LOWBIT_BASE >> 2).all()
                distinct = np.array([len(np.unique(r)) for r in w.reshape(-1, k)])
                assert (distinct >= 2).mean() > 0.7 and (distinct >= 3).any()
        # the complex forms keep ties: half the phasors are exact
        zt = I.magnitudes(I.make("ties", shape, 2, True))
        assert (bits(zt) == bits(t)).mean() > 0.45
        zl = bits(I.magnitudes(I.make("lowbit", shape, 2, True)))
        assert (zl == bits(lo)).mean() > 0.45 and (np.abs(zl.astype(np.int64) - I.LOWBIT_BASE) <= 8).all()


def test_nan_class_has_nan_medians_and_windows_with_nans_above_the_rank():
    for shape in I.CLASS_SHAPES:
        for is_complex in (False, True):
            a = I.make("nan", shape, 3, is_complex)
            m = I.magnitudes(a)
            isn = np.isnan(m)
            if not is_complex:
                assert (bits(m)[isn] == I.NAN_BITS).all() and 0.08 < isn.mean() < 0.45
            assert isn[shape[0] // 2].all() and isn[:, shape[1] // 3].all()
            for kh, kp in I.KERNEL_PAIRS[1:]:
                for k, axis in ((kh, 0), (kp, 1)):
                    w = windows(m, k, axis)
                    n_nan = np.isnan(w).sum(axis=-1)
                    med = np.sort(w, axis=-1)[..., k // 2]
                    assert np.array_equal(np.isnan(med), n_nan >= k - k // 2)           # a NaN ranks above everything else
                    assert np.isnan(med).any(), (shape, k, axis)                         # the rank-k//2 element is a NaN
                    if k > 2:
                        assert ((n_nan > 0) & ~np.isnan(med)).any(), (shape, k, axis)    # NaNs in the window, all above the rank
                    assert np.array_equal(bits(hpss_np.median_reflect(m, k, axis)), bits(np.moveaxis(med, -1, axis)))
    w = I.make("wide", (67, 66), 3, True)
    assert np.isinf(I.magnitudes(w)).any() and np.isnan(I.magnitudes(w)).any()


def test_numpy_on_the_complex_special_cells():
    """np.abs of a complex64 with an infinite part is inf, whatever the other part (NaN included); with a NaN part and no infinite
    one it is NaN.  The planted kinds are all present at the class shapes."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    z = np.array([complex(nan, 2), complex(2, nan), complex(inf, 2), complex(-inf, 2), complex(2, inf), complex(2, -inf), complex(inf, nan),
                  complex(nan, -inf), complex(nan, nan)], np.complex64)
    m = I.magnitudes(z)
    assert np.array_equal(np.isnan(m), [True, True, False, False, False, False, False, False, True])
    assert (m[2:8] == inf).all()
    for shape in I.CLASS_SHAPES:
        for cls in ("wide", "nan"):
            z = I.to_complex(I.make(cls, shape, 4), 4)
            plain = z.copy()
            kind = I.plant_special_cells(z, 4)
            assert set(np.unique(kind)) == set(range(-1, len(I.SPECIAL_PARTS))), (shape, cls)
            m = I.magnitudes(z)
            has_inf = np.isinf(z.real) | np.isinf(z.imag)
            has_nan = np.isnan(z.real) | np.isnan(z.imag)
            assert np.isinf(m)[has_inf].all() and np.array_equal(np.isnan(m), has_nan & ~has_inf)
            over = np.isinf(m) & ~has_inf                                   # finite parts whose modulus is past FLT_MAX
            assert (np.hypot(z.real[over].astype(np.float64), z.imag[over].astype(np.float64)) > 3.4028e38).all()
            assert np.array_equal(cells(z)[kind < 0], cells(plain)[kind < 0])
            made = I.make(cls, shape, 4, True)                              # `nan` puts its NaN frame and bin back on top
            rest = np.ones(shape, bool)
            if cls == "nan":
                rest[shape[0] // 2, :] = rest[:, shape[1] // 3] = False
                assert np.isnan(I.magnitudes(made)[~rest]).all()
            assert np.array_equal(cells(made)[rest], cells(z)[rest])
            assert set(np.unique(kind[rest])) == set(range(-1, len(I.SPECIAL_PARTS))), (shape, cls)
    # numpy's product of a complex64 with a float32 mask is the complex product with mask + 0i: an infinite or NaN part reaches
    # both parts of the result through its product with the 0
    with np.errstate(all="ignore"):
        p = np.array([complex(inf, 2), complex(2, -inf), complex(nan, 2), complex(-1, -2)], np.complex64) * np.float32([1, 0.5, 1, 0])
    assert p[0].real == inf and np.isnan(p[0].imag) and np.isnan(p[1].real) and p[1].imag == -inf and np.isnan(p[2].real) and np.isnan(p[2].imag)
    assert np.array_equal(bits(p[3:]), bits(np.float32([0.0, -0.0])))      # (-1 * 0) - (-2 * 0) = -0 - -0 = +0; (-1 * 0) + (-2 * 0) = -0
    assert np.array_equal(bits(product_np(np.array([complex(inf, 2), complex(2, -inf), complex(nan, 2), complex(-1, -2)], np.complex64),
                                          np.float32([1, 0.5, 1, 0])))[6:], bits(p)[6:])


def product_np(spec, mask):
    """numpy's spec * mask written out part by part.  complex64: the product with mask + 0i as numpy's vector loop forms it,
    re = fma(re, mask, -(im * 0)), im = fma(re, 0, im * mask) = re * 0 + im * mask: the cross products with the 0 turn an
    infinite or NaN part into a NaN in both parts and decide the sign of a zero; the fused real part keeps the sign of a product
    that underflows, the imaginary part's product is rounded before the sum.  (The real part's addend is a zero, an infinity or
    a NaN, so the float64 sum below is the fused result before its one rounding.)"""
    spec, mask = np.asarray(spec), np.asarray(mask, np.float32)
    with np.errstate(all="ignore"):
        if not np.iscomplexobj(spec):
            return spec * mask
        zero = np.zeros_like(mask)
        m = mask.astype(np.float64)
        out = np.empty(spec.shape, np.complex64)
        out.real = (spec.real.astype(np.float64) * m - (spec.imag * zero).astype(np.float64)).astype(np.float32)
        out.imag = spec.real * zero + spec.imag * mask
    return out


def test_numpys_complex_product_is_the_fused_form_with_a_zero_imaginary_mask():
    """what `spec * mask` means cell by cell, on every class's complex form and masks of every kind"""
    rng = np.random.default_rng(6)
    for cls in I.COMPLEX_CLASSES:
        z = I.make(cls, (67, 66), 6, True)
        for mask in (rng.random(z.shape, dtype=np.float32), (rng.random(z.shape) < 0.5).astype(np.float32),
                     np.where(rng.random(z.shape) < 0.1, np.float32(np.nan), np.float32(0.5))):
            with np.errstate(all="ignore"):
                want = z * mask
            got = product_np(z, mask)
            wn, gn = np.isnan(want.view(np.float32)), np.isnan(got.view(np.float32))
            assert np.array_equal(wn, gn), cls
            assert np.array_equal(bits(want)[~wn], bits(got)[~gn]), cls


def test_pair_table_puts_every_listed_pair_where_the_gpu_test_expects_it():
    pairs = I.mask_pairs()
    assert pairs.shape == (I.N_PAIRS, 2) and pairs.dtype == np.float32 and I.N_PAIRS > 64 and I.PAIR_LINES > 64
    listed = I.f32(np.array(I.LISTED_PAIRS_BITS, np.uint32))
    assert np.array_equal(bits(pairs[:len(listed)]), bits(listed))
    tiny, fmax, inf = np.float32(hpss_np.TINY), np.finfo(np.float32).max, np.float32(np.inf)
    text = [tuple("nan" if np.isnan(v) else float(v) for v in p) for p in listed]
    for want in ((0.0, 0.0), (float(tiny), 0.0), (float(np.nextafter(tiny, np.float32(0))), 0.0), (float(tiny), float(np.nextafter(tiny, np.float32(0)))),
                 (0.75, 0.75), (0.75, float(np.nextafter(np.float32(0.75), np.float32(1)))), (float(fmax), float(fmax / np.float32(2))),
                 (float(inf), 1.0), (1.0, float(inf)), (float(inf), float(inf)), ("nan", 0.0), (0.0, "nan"), ("nan", 1.0), (1.0, "nan"),
                 ("nan", "nan"), ("nan", float(inf)), (1.0, float(np.float32(1e-30))), (1.0, 2.0 ** -20)):
        assert want in text, want
    sub = listed[1]
    assert (sub > 0).all() and (sub < tiny).all() and sub[0] != sub[1]                  # two subnormals
    with np.errstate(over="ignore"):
        assert fmax * np.float32(3) == inf and (fmax / np.float32(2)) * np.float32(2) == fmax
    rest = pairs[len(listed):]
    assert np.isfinite(rest).all() and (rest > 0).all() and len(np.unique(np.floor(np.log2(rest[:, 0] / rest[:, 1])))) > 12
    for transposed, kernel in ((False, (3, 1)), (True, (1, 3))):
        t = I.pair_table(pairs, transposed)
        assert t.shape == ((I.N_PAIRS, I.PAIR_LINES) if transposed else (I.PAIR_LINES, I.N_PAIRS)) and t.dtype == np.float32
        harm, perc = hpss_np.median_reflect(t, kernel[0], 0), hpss_np.median_reflect(t, kernel[1], 1)
        eh, ep = I.pair_table_expected(pairs, transposed)
        assert np.array_equal(bits(harm), bits(eh)) and np.array_equal(bits(perc), bits(ep))
        if transposed:
            harm, perc = perc.T, harm.T                                                 # roles swapped: back to (u, own value)
        is_v = np.arange(I.PAIR_LINES) % 3 == 2
        assert is_v.sum() == 22 and not is_v[-1]
        for c in range(I.N_PAIRS):
            assert (bits(harm[:, c]) == bits(pairs[c, :1])).all()
            assert (bits(perc[is_v, c]) == bits(pairs[c, 1:])).all() and (bits(perc[~is_v, c]) == bits(pairs[c, :1])).all()


def test_mask64_and_numpys_float32_mask_on_the_pair_table():
    """E_np, the distance of numpy's float32 route (square, square root or `**`, float32 sum and quotient) from the float64
    statement, is measured per power and printed; the NaN patterns agree, every NaN pair gives a NaN mask and the branch edges
    give what the rule says"""
    pairs = I.mask_pairs()
    harm, perc = I.pair_table_expected(pairs)
    worst = {}
    for power in I.POWERS_EXACT + I.POWERS_GENERAL:
        for margin in I.MARGINS:
            one = margin == (1.0, 1.0)
            with np.errstate(all="ignore"):
                sides = ((harm, perc * np.float32(margin[0])), (perc, harm * np.float32(margin[1])))
            for x, xref in sides:
                m32, m64 = hpss_np.mask(x, xref, power, one), hpss_np.mask64(x, xref, power, one)
                if np.isinf(power):
                    assert m32.dtype == bool and np.array_equal(m32, m64) and not m32[np.isnan(x) | np.isnan(xref)].any()
                    continue
                assert m32.dtype == m64.dtype == np.float32
                nan_in = np.isnan(x) | np.isnan(xref)
                assert np.isnan(m32[nan_in]).all() and np.isnan(m64[nan_in]).all() and nan_in.sum() >= 6 * 22
                same_nan, d = hpss_np.ulp_distance_nan(m32, m64)
                assert same_nan
                worst[power] = max(worst.get(power, 0), d)
                small = np.maximum(x, xref) < hpss_np.TINY
                assert small.any() and (m64[small] == (0.5 if one else 0.0)).all()
    print("\nE_np, float32 ulp of hpss_np.mask from the float64 mask on the pair table, by power:", worst)
    assert set(worst) == set(I.POWERS_EXACT[:1] + I.POWERS_EXACT[2:] + I.POWERS_GENERAL)
    # the edges, one by one (harm, perc) -> mask_h at margins (1, 1), power 2
    m = hpss_np.mask64(pairs[:, 0], pairs[:, 1], 2.0, True)
    tiny = np.float32(hpss_np.TINY)
    assert m[0] == 0.5 and m[1] == 0.5 and m[3] == 0.5                      # Z = 0, subnormal, one bit below FLT_MIN
    assert m[2] == 1.0 and m[4] != 0.5 and 0.5 < m[4] < 0.51                # Z = FLT_MIN exactly: the formula
    assert m[5] == 0.5 and m[6] < 0.5 and np.isnan(m[8]) and np.isnan(m[9]) and np.isnan(m[10])
    assert m[17] == 1.0 and 0 < hpss_np.mask64(pairs[17:18, 1], pairs[17:18, 0], 1.5, True)[0] < tiny      # the power underflows
    assert hpss_np.mask64(pairs[17:18, 1], pairs[17:18, 0], 3.0, True)[0] == 0
    with np.errstate(all="ignore"):
        assert np.isnan(hpss_np.mask64(pairs[7:8, 1], pairs[7:8, 0] * np.float32(3), 2.0, False))[0]      # Xref = inf: 0 / (0 + NaN)
        assert hpss_np.mask64(pairs[7:8, 0], pairs[7:8, 1] * np.float32(2), 40.0, False)[0] == 0.5         # X == Xref
    assert not hpss_np.mask64(pairs[5:6, 0], pairs[5:6, 1], np.inf, True)[0]                               # hard mask, X == Xref
