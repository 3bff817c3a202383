"""The seven entry points of csrc/expander.hip (ABI 107, and par_mean_mag_frames_f32 of ABI 108) at the C ABI, cell by cell, against
the oracles and bounds of tests/expander_np.py -- where expander.* and spectrum_flat.* (one tape, hop 64) do not reach: hop 1, hops
above the 1024-sample tile and hops that are no power of two, a signal that runs past the curve, a single frame, pitched magnitude
rows, zero frames, the stride loop of k_absmax / k_div, smoothing windows on data where a plain running sum drifts.

Every device buffer lies between guard rows and the kernel gets an interior pointer; each test ends by checking its guards bit for
bit.  tests/test_expander_kernels_cpu.py proves the bounds with the reference alone.  pytest -s prints the measured figures
(NOTES.md, Spectral Expander)."""
import ctypes

import numpy as np
import pytest

import expander_np as E
from test_heal_kernels_gpu import BIT_EQUAL_SHARE, Guarded, bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def par():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pyaudiorestoration_amd import _dev, _lib

    class P:
        pass
    p = P()
    p.torch, p.dev, p.L, p.check, p.stream = torch, 0, _lib.lib(), _lib.check, lambda: _dev.stream_ptr(0)
    p.scratch_bytes = _lib.NORMALIZE_SCRATCH_BYTES
    return p


# ------------------------------------------------------------------------------------------ frame sums
def frame_sums(par, fn, mag, frames, bins, pitched, acc0, db):
    """two chunk calls of `frames` frames on one acc -> worst error as a share of the bound (each call against its own bound,
    the second starting from the device's first result)"""
    pitch = bins + E.MEAN_PAD if pitched else bins
    body = np.full((2 * frames, pitch), E.MAG_SENTINEL, dtype=np.float32)
    body[:, :bins] = mag
    m = Guarded(par, body, 2, E.MAG_SENTINEL)
    acc = Guarded(par, acc0, 16, -1234.5)
    worst, start = 0.0, np.array(acc0)
    for chunk in range(2):
        par.check(fn(par.dev, m.ptr(chunk * frames * pitch), frames, bins, pitch if pitched else 0, acc.ptr(), par.stream()))
        par.torch.cuda.synchronize()
        got = acc.read().copy()
        with np.errstate(all="ignore"):
            ref, bound = E.frame_sum_np(mag[chunk * frames:(chunk + 1) * frames], start, db)
        if frames == 0:
            assert np.array_equal(bits(got), bits(acc0))
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
        err = np.abs(got[fin] - ref[fin])
        bad = np.flatnonzero(~(err <= bound[fin]))
        assert len(bad) == 0, (frames, bins, pitched, chunk, bad[:5].tolist(), err[bad[:5]], bound[fin][bad[:5]])
        if frames and fin.any():
            worst = max(worst, float(np.max(err / bound[fin])))
        start = got
    assert acc.guards_intact() and m.unchanged()
    return worst


@pytest.mark.parametrize("db", [True, False])
@pytest.mark.parametrize("bins", E.MEAN_BINS)
def test_frame_sums(par, bins, db):
    fn = par.L.par_mean_db_frames_f32 if db else par.L.par_mean_mag_frames_f32
    worst = 0.0
    for frames in E.MEAN_FRAMES:
        mag, acc0 = E.mean_case(bins, frames)
        for pitched in (False, True):
            worst = max(worst, frame_sums(par, fn, mag, frames, bins, pitched, acc0, db))
    print(f"\nframe sums ({'dB' if db else 'magnitude'}), {bins} bins: worst error {worst:.3f} of the bound")


@pytest.mark.parametrize("db", [True, False])
def test_frame_sums_zero_and_nan(par, db):
    """a zero magnitude makes the dB sum of its bin -inf (and leaves a magnitude sum alone), a NaN makes either NaN; the
    neighbouring bins keep their bounds"""
    fn = par.L.par_mean_db_frames_f32 if db else par.L.par_mean_mag_frames_f32
    mag, acc0 = E.mean_case(65, 5)
    mag = np.array(mag)
    mag[2, 5], mag[8, 5], mag[3, 7] = 0.0, 0.0, np.nan
    frame_sums(par, fn, mag, 5, 65, True, acc0, db)
    with np.errstate(all="ignore"):
        ref, _ = E.frame_sum_np(mag[:5], acc0, db)
    assert (ref[5] == -np.inf) == db and np.isnan(ref[7]) and np.isfinite(np.delete(ref, [5, 7])).all()


# ------------------------------------------------------------------------------------------ uniform filter
@pytest.mark.parametrize("n", E.UF_N)
def test_uniform_filter_nearest(par, n):
    x = E.uf_case(n)
    src = Guarded(par, x, 1, 1e300)
    for size in E.uf_sizes(n):
        out = Guarded(par, np.full((E.UF_ROWS, n), -1234.5), 1, -1234.5)
        par.check(par.L.par_uniform_filter_nearest_f64(par.dev, src.ptr(), E.UF_ROWS, n, size, out.ptr(), par.stream()))
        par.torch.cuda.synchronize()
        got = out.read().copy()
        ref, bound = E.uniform_nearest_np(x, size), E.uniform_bound(x, size)
        err = np.abs(got - ref)
        bad = np.argwhere(~(err <= bound))
        assert len(bad) == 0, (n, size, len(bad), bad[:5].tolist())
        same = int(np.sum(bits(got) == bits(ref)))
        print(f"\nuniform n={n} size={size}: worst error {float(np.max(err / bound)):.3f} of the bound by row "
              f"{np.round(np.max(err / bound, axis=1), 3).tolist()}; {same} of {got.size} outputs equal the exact mean rounded once")
        assert out.guards_intact()
    assert src.unchanged()


# ------------------------------------------------------------------------------------------ expander gain
@pytest.mark.parametrize("hop,n,frames", E.GAIN_SHAPES)
def test_expand_gain(par, hop, n, frames):
    for n_ch in E.GAIN_CHANNELS:
        sig, curve = E.gain_case(hop, n, frames, n_ch)
        stride = n_ch + 2
        ref, bound = E.expand_gain_np(sig, curve, hop)
        reach = E.nan_reach(curve, hop, n)
        s = Guarded(par, sig, 4, np.float32(7e37))
        cv = Guarded(par, curve, 1, 1e300)

        def call(o32, o64):
            par.check(par.L.par_expand_gain_f32(par.dev, s.ptr(), stride, n_ch, n, cv.ptr(), frames, hop, E.CLIP_LO, E.CLIP_HI, o32.ptr(),
                                                stride, o64.ptr() if o64 is not None else None, par.stream()))
            par.torch.cuda.synchronize()
        # ---- float64 outputs: [boosted, float64(sig)] x channels x n
        o32 = Guarded(par, np.full((n, stride), np.float32(-1234.5)), 4, np.float32(-1234.5))
        o64 = Guarded(par, np.full((2 * n_ch, n), -1234.5), 1, -1234.5)
        call(o32, o64)
        got = o64.read().copy()
        assert np.array_equal(np.isnan(got[:n_ch]), reach), (n_ch, np.argwhere(np.isnan(got[:n_ch]) != reach)[:5].tolist())
        assert np.isfinite(got[:n_ch][~reach]).all()
        err = np.abs(got[:n_ch] - ref)
        bad = np.argwhere(~(err <= bound) & ~reach)
        assert len(bad) == 0, (n_ch, len(bad), bad[:5].tolist())
        assert np.array_equal(bits(got[n_ch:]), bits(sig[:, :n_ch].T.astype(np.float64)))           # the low-pass input: the channel itself
        assert o32.unchanged() and o64.guards_intact()
        with np.errstate(invalid="ignore", divide="ignore"):
            share = float(np.max(np.where(bound > 0, err / bound, 0.0)[~reach], initial=0.0))
        # ---- float32 output, interleaved
        o32 = Guarded(par, np.full((n, stride), np.float32(-1234.5)), 4, np.float32(-1234.5))
        call(o32, None)
        g32 = o32.read().copy()
        assert np.all(bits(g32[:, n_ch:]) == bits(np.float32(-1234.5)))                             # the stride's spare columns
        g32 = g32[:, :n_ch].T
        with np.errstate(invalid="ignore"):
            r32 = ref.astype(np.float32)
        assert np.array_equal(np.isnan(g32), reach) and np.isfinite(g32[~reach]).all()
        ok = ~reach
        assert np.all(np.abs(g32[ok].astype(np.float64) - r32[ok]) <= np.spacing(np.abs(r32[ok])))
        equal = int(np.sum(bits(g32[ok]) == bits(r32[ok])))
        assert equal >= BIT_EQUAL_SHARE * ok.sum(), (equal, int(ok.sum()))
        assert o32.guards_intact() and s.unchanged() and cv.unchanged()
        print(f"\nexpand gain hop={hop} n={n} frames={frames} ch={n_ch}: float64 worst {share:.3f} of the bound, {int(reach.sum())} NaN cells; "
              f"float32 {equal} of {int(ok.sum())} bit-equal to float32(ref)")


# ------------------------------------------------------------------------------------------ sum rows
@pytest.mark.parametrize("n", E.SUM_N)
def test_sum_rows(par, n):
    for n_ch in E.GAIN_CHANNELS:
        a, b = E.sum_case(n, n_ch)
        ga, gb = Guarded(par, a, 1, 1e300), Guarded(par, b, 1, -1e300)
        out = Guarded(par, np.full((n, n_ch + 1), np.float32(-1234.5)), 8, np.float32(-1234.5))
        par.check(par.L.par_sum_rows_f64_f32(par.dev, ga.ptr(), gb.ptr(), n_ch, n, out.ptr(), n_ch + 1, par.stream()))
        par.torch.cuda.synchronize()
        want = np.full((n, n_ch + 1), np.float32(-1234.5))
        want[:, :n_ch] = np.float32(a + b).T
        assert np.array_equal(bits(out.read()), bits(want)), (n, n_ch)
        assert out.guards_intact() and ga.unchanged() and gb.unchanged()


# ------------------------------------------------------------------------------------------ normalize
def normalize(par, d):
    buf = Guarded(par, d, 256, np.float32(9e37))
    scratch = Guarded(par, np.full(par.scratch_bytes // 4, np.float32(-5.5)), 64, np.float32(-5.5))
    par.check(par.L.par_normalize_f32(par.dev, buf.ptr(), len(d), scratch.ptr(), par.stream()))
    par.torch.cuda.synchronize()
    got = buf.read().copy()
    assert buf.guards_intact() and scratch.guards_intact()
    return got


@pytest.mark.parametrize("count", E.NORM_COUNTS)
def test_normalize(par, count):
    for at in E.norm_positions(count):
        d = E.norm_case(count, at)
        got = normalize(par, d)
        want = E.normalize_np(d)
        assert got[at] == np.float32(-1.0)
        assert np.array_equal(bits(got), bits(want)), (count, at, np.flatnonzero(bits(got) != bits(want))[:5].tolist())
    d = np.array(E.norm_case(count, 0))
    d[count // 2] = np.nan                                           # a NaN anywhere: everything NaN, as np.max gives NaN
    assert np.isnan(normalize(par, d)).all()
    zeros = np.zeros(min(count, 4097), np.float32)
    assert np.isnan(normalize(par, zeros)).all()                     # 0 / 0, as numpy


# ------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(par):
    L, dev, p = par.L, par.dev, ctypes.c_void_p(8)
    for fn in (L.par_mean_db_frames_f32, L.par_mean_mag_frames_f32):
        assert fn(dev, None, 3, 5, 0, p, None) == 1 and fn(dev, p, 3, 5, 0, None, None) == 1
        assert fn(dev, p, -1, 5, 0, p, None) == 1 and fn(dev, p, 3, 0, 0, p, None) == 1 and fn(dev, p, 3, 5, 4, p, None) == 1
        assert fn(dev, p, 0, 5, 0, p, None) == 0                                            # no frames: nothing to do
    uf = L.par_uniform_filter_nearest_f64
    q = ctypes.c_void_p(16)
    assert uf(dev, None, 1, 5, 3, q, None) == 1 and uf(dev, p, 1, 5, 3, None, None) == 1 and uf(dev, p, 1, 5, 3, p, None) == 1
    assert uf(dev, p, 0, 5, 3, q, None) == 1 and uf(dev, p, 1, 0, 3, q, None) == 1
    assert uf(dev, p, 1, 5, 4, q, None) == 1 and uf(dev, p, 1, 5, 0, q, None) == 1        # even, empty
    eg = L.par_expand_gain_f32
    assert eg(dev, None, 1, 1, 5, p, 3, 2, -120.0, -85.0, p, 1, None, None) == 1
    assert eg(dev, p, 1, 1, 5, None, 3, 2, -120.0, -85.0, p, 1, None, None) == 1
    assert eg(dev, p, 1, 1, 5, p, 3, 2, -120.0, -85.0, None, 1, None, None) == 1           # neither output
    assert eg(dev, p, 1, 1, 0, p, 3, 2, -120.0, -85.0, p, 1, None, None) == 1
    assert eg(dev, p, 1, 1, 5, p, 0, 2, -120.0, -85.0, p, 1, None, None) == 1
    assert eg(dev, p, 1, 1, 5, p, 3, 0, -120.0, -85.0, p, 1, None, None) == 1              # hop = 0
    assert eg(dev, p, 1, 2, 5, p, 3, 2, -120.0, -85.0, p, 2, None, None) == 1              # sig_stride < channels
    assert eg(dev, p, 2, 2, 5, p, 3, 2, -120.0, -85.0, p, 1, None, None) == 1              # out_stride < channels
    sr = L.par_sum_rows_f64_f32
    assert sr(dev, None, p, 1, 5, p, 1, None) == 1 and sr(dev, p, None, 1, 5, p, 1, None) == 1 and sr(dev, p, p, 1, 5, None, 1, None) == 1
    assert sr(dev, p, p, 0, 5, p, 1, None) == 1 and sr(dev, p, p, 1, 0, p, 1, None) == 1 and sr(dev, p, p, 2, 5, p, 1, None) == 1
    nm = L.par_normalize_f32
    assert nm(dev, None, 5, p, None) == 1 and nm(dev, p, 5, None, None) == 1 and nm(dev, p, 0, p, None) == 1
