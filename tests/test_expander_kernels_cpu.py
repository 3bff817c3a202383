"""Preconditions of tests/test_expander_kernels_gpu.py, on the CPU: the oracles of tests/expander_np.py against numpy and scipy on
the same inputs, and the stated bounds against the reference alone -- a float64 evaluation in the kernel's documented order keeps
each bound, so a kernel that breaks one is wrong, and the defect each bound exists for (a dropped frame, a plain running sum)
breaks it.  pytest -s prints the measured figures (NOTES.md, Spectral Expander)."""
import math

import numpy as np
import pytest
import scipy.ndimage

import expander_np as E


# ------------------------------------------------------------------------------------------ frame sums
def _lane_order_sum(t, acc0):
    """float64 in k_mean_db_frames' order: four lanes over every 4th frame, joined in lane order, then added to acc"""
    lanes = [0.0] * 4
    for f in range(len(t)):
        lanes[f % 4] += float(t[f])
    s = lanes[0]
    for v in lanes[1:]:
        s += v
    return float(acc0) + s


@pytest.mark.parametrize("db", [True, False])
def test_frame_sum_oracle_and_bound(db):
    worst = 0.0
    for bins in E.MEAN_BINS:
        for frames in E.MEAN_FRAMES:
            mag, acc0 = E.mean_case(bins, frames)
            assert mag.shape == (2 * frames, bins) and np.all(acc0 != 0)
            if frames:
                assert 1e-6 <= mag.min() and mag.max() <= 1e-1 + 1e-8
            chunk = mag[:frames]
            ref, bound = E.frame_sum_np(chunk, acc0, db)
            t = E.frame_terms(chunk, db)
            assert np.allclose(ref, acc0 + t.sum(axis=0), rtol=1e-12, atol=0)               # numpy's own sum, pairwise
            got = np.array([_lane_order_sum(t[:, b], acc0[b]) for b in range(bins)])
            if frames == 0:
                assert np.array_equal(ref, acc0) and np.array_equal(got, acc0)
                continue
            assert np.all(np.abs(got - ref) <= bound)                                       # the kernel's order keeps the bound
            worst = max(worst, float(np.max(np.abs(got - ref) / bound)))
            # a dropped frame moves a dB sum by at least 20 dB, a magnitude sum by at least 1e-6: far outside the bound
            dropped = np.array([_lane_order_sum(t[1:, b], acc0[b]) for b in range(bins)])
            assert np.all(np.abs(dropped - ref) >= (20.0 if db else 1e-6) - 1e-9) and np.all(np.abs(dropped - ref) > 1e5 * bound)
    print(f"\nframe sums ({'dB' if db else 'magnitude'}): the lane order reaches {worst:.3f} of the bound")


def test_frame_sum_special_values():
    mag = np.array(E.mean_case(65, 5)[0][:5])
    mag[2, 5], mag[3, 7] = 0.0, np.nan
    ref, _ = E.frame_sum_np(mag, np.ones(65), True)
    assert ref[5] == -np.inf and np.isnan(ref[7]) and np.isfinite(np.delete(ref, [5, 7])).all()
    ref, _ = E.frame_sum_np(mag, np.ones(65), False)
    assert np.isfinite(ref[5]) and np.isnan(ref[7])


# ------------------------------------------------------------------------------------------ uniform filter
def _neumaier(x, size):
    """k_uniform_nearest in Python floats: Neumaier's running sum on the kernel's schedule"""
    rows, n = x.shape
    h, seg = size // 2, max(size, E.UF_SEG)
    out = np.empty_like(x)
    for r in range(rows):
        row = x[r].tolist()

        def at(q):
            return row[0 if q < 0 else (n - 1 if q >= n else q)]
        for i0 in range(0, n, seg):
            s = c = 0.0

            def add(v):
                nonlocal s, c
                t = s + v
                c += (s - t) + v if abs(s) >= abs(v) else (v - t) + s
                s = t
            for q in range(i0 - h, i0 + h + 1):
                add(at(q))
            out[r, i0] = (s + c) / size
            for i in range(i0 + 1, min(i0 + seg, n)):
                add(at(i + h))
                add(-at(i - h - 1))
                out[r, i] = (s + c) / size
    return out


@pytest.mark.parametrize("n", [1, 2, 255, 257])
def test_uniform_oracle_equals_fsum_and_scipy(n):
    x = E.uf_case(n)
    assert x.shape == (E.UF_ROWS, n)
    for size in E.uf_sizes(n):
        ref = E.uniform_nearest_np(x, size)
        by_fsum = E.uniform_nearest_fsum(x, size)
        assert np.all(np.abs(ref - by_fsum) <= np.spacing(np.abs(ref)))                     # fsum / size rounds twice, the oracle once
        sc = scipy.ndimage.uniform_filter1d(x[2], size, mode="nearest")
        assert np.max(np.abs(sc - ref[2])) <= 1e-9                                          # the well-conditioned row
        k = n // 2
        assert ref[0, k] == float(E.fraction_mean(x[0, np.clip(np.arange(k - size // 2, k + size // 2 + 1), 0, n - 1)]))


@pytest.mark.parametrize("n,sizes", [(255, (1, 3, 255, 257, 511)), (257, (1, 3, 255, 257, 513)), (1000, (1, 3, 255, 513, 2001)),
                                     (20001, (257,))])
def test_uniform_bound_holds_for_compensated_sums_and_breaks_a_running_sum(n, sizes):
    x = E.uf_case(n)
    for size in sizes:
        ref, bound = E.uniform_nearest_np(x, size), E.uniform_bound(x, size)
        comp = np.abs(_neumaier(x, size) - ref) / bound
        plain = np.abs(E.uniform_running_sum(x, size) - ref) / bound
        print(f"\nuniform n={n} size={size}: compensated sums reach {comp.max():.3f} of the bound; a running sum "
              f"{plain[0].max():.3g} (row 0), {plain[1].max():.3g} (row 1), {plain[2].max():.3g} (row 2)")
        assert comp.max() <= 1.0
        if size < n:                                                # some sample leaves the window inside a segment
            assert plain[:2].max() > 1.0, (n, size)
        assert np.max(np.abs(scipy.ndimage.uniform_filter1d(x[2], size, mode="nearest") - ref[2])) <= 1e-9


# ------------------------------------------------------------------------------------------ expander gain
@pytest.mark.parametrize("hop,n,frames", E.GAIN_SHAPES)
def test_gain_oracle_and_its_roundings(hop, n, frames):
    for n_ch in E.GAIN_CHANNELS:
        sig, curve = E.gain_case(hop, n, frames, n_ch)
        fin = curve[np.isfinite(curve)]
        assert fin.min() < E.CLIP_LO < E.CLIP_HI < fin.max() or frames < 8
        if frames >= 30:
            assert (curve == E.CLIP_LO).any() and (curve == E.CLIP_HI).any()
        assert np.isnan(curve).sum() == (n_ch if frames >= 3 else 0)
        ref, bound = E.expand_gain_np(sig, curve, hop)
        fac = E.gain_factors(curve)
        assert np.nanmin(fac) >= 1.0 and np.nanmax(fac) <= 10 ** (35 / 20) * (1 + 1e-15)
        reach = E.nan_reach(curve, hop, n)
        assert np.array_equal(np.isnan(ref), reach)                                          # np.interp's own NaNs, nothing else
        # on a frame the factor itself; past the curve its last value
        for c in range(n_ch):
            on = np.arange(0, min(n, (frames - 1) * hop + 1), hop)
            assert np.array_equal(ref[c, on], sig[on, c].astype(np.float64) * fac[c, on // hop], equal_nan=True)
            past = np.arange((frames - 1) * hop, n)
            assert np.array_equal(ref[c, past], sig[past, c].astype(np.float64) * fac[c, -1], equal_nan=True)
        # float32(ref) is decided by the float64 error bound in all but a vanishing share of the cells
        ok = ~reach
        with np.errstate(invalid="ignore"):
            moved = (ref - bound).astype(np.float32)[ok] != (ref + bound).astype(np.float32)[ok]
        assert moved.mean() <= 1e-4, moved.mean()
        assert np.all(bound[ok] <= 2e-15 * 57 * np.abs(sig[:, :n_ch].T.astype(np.float64))[ok])


def test_gain_shapes_cover_what_they_are_for():
    shapes = E.GAIN_SHAPES
    assert any(hop == 1 and frames > n for hop, n, frames in shapes)                        # the curve outlasts the signal
    assert any(n > (frames - 1) * hop + 1024 for hop, n, frames in shapes)                  # a whole tile past the curve
    assert any(hop > 1024 for hop, n, frames in shapes) and any(hop & (hop - 1) for hop, n, frames in shapes)
    assert any(frames == 1 for hop, n, frames in shapes)


# ------------------------------------------------------------------------------------------ sum rows, normalize
def test_sum_and_normalize_oracles():
    a, b = E.sum_case(257, 3)
    s = np.float32(a + b)
    assert s[0, 0] == np.float32(1.0) and s[0, 1] == np.float32(1.0 + 2.0 ** -22)            # the ties go to even
    for count in E.NORM_COUNTS[:-1]:
        for at in E.norm_positions(count):
            d = E.norm_case(count, at)
            out = E.normalize_np(d)
            assert out[at] == np.float32(-1.0) and np.max(np.abs(out)) == 1.0
    assert E.norm_positions(E.NORM_COUNTS[-1])[1] >= E.NORM_GRID_SPAN and len(E.norm_positions(E.NORM_COUNTS[-1])) == 3
    assert np.isnan(E.normalize_np(np.zeros(5, np.float32))).all()
    d = np.array(E.norm_case(255, 0))
    d[100] = np.nan
    assert np.isnan(E.normalize_np(d)).all()
    assert math.isclose(float(E.NORM_PEAK), -7.5)
