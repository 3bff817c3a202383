"""par_piptrack_f32, par_track_corr_f64 and par_zero_crossings_f64 at the C ABI, on the GPU, against the numpy statements of
tests/track_abi_inputs.py (whose cases tests/test_track_abi_inputs_cpu.py proves to drive the paths they are named for).

Piptrack: pitches and magnitudes equal the float32 statement bit for bit, on every cell of every case; nothing is exempt.
Correlation: the resampled rows R equal the statement bit for bit on the integer cases, ties pick the statement's lag, the NaN masks
are equal, a peak on the last lag is PAR_ERR_INDEX; `changes` and log2(freqs) stay within a measured bound under the 1e-9 cap.
Zero crossings: numpy's indices on signed zeros, subnormals, NaN and infinities.  Every output buffer starts as NaN (or -1) with
guard cells behind it; pytest -s prints the measured errors (NOTES.md, K_track)."""
import ctypes

import numpy as np
import pytest

import track_abi_inputs as T

pytestmark = pytest.mark.gpu

SAME_MAG_TOL = 1e-9            # the cap: tests/test_trackers_gpu.py's bound for this tracker.  Both sides are float64 evaluations of the
#                                same numbers (summation order, where the norm is divided, libm's exp2 / log2): each bound below is
#                                10 x the worst measured on the MI355X over its cases, and must stay under the cap
CORR_TOL_INTEGER = 3.6e-14     # lags; |changes - statement| and |log2 freqs - cumsum|, integer cases: measured 3.55e-15 (one ulp of a
#                                value between 16 and 32 lags; the placed-bump cases, ties included, measure 0)
CORR_TOL_REALISTIC = 6.4e-12   # lags; the same two on the realistic cases: measured 6.39e-13 (nb 33: a broad peak, curvature 1e-3)
CORR_TOL_ROWS = 5.6e-15        # of max |R|; the realistic cases' resampled rows: measured 5.55e-16 (the integer cases' are bit-identical)
GUARD = 16


@pytest.fixture(scope="module")
def par():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    from pyaudiorestoration_amd import _dev, _lib

    class P:
        pass
    p = P()
    p.torch, p.dev, p.L, p.lib, p.stream = torch, 0, _lib.lib(), _lib, lambda: _dev.stream_ptr(0)
    return p


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def up(par, a):
    return par.torch.from_numpy(np.array(a, order="C")).cuda()           # a copy: the cases' arrays are read-only


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def ulps32(a, b):
    """distance in float32 steps between finite arrays of one sign pattern (0 where equal)"""
    ia, ib = bits(a).astype(np.int64), bits(b).astype(np.int64)
    return np.abs(ia - ib)


# ================================================================================================ piptrack
def run_piptrack(par, c):
    t = par.torch
    mag_t = up(par, c.mag)
    cells = c.frames * c.bins
    outs = [t.full((cells + GUARD,), float("nan"), dtype=t.float32, device="cuda") for _ in range(2)]
    rc = par.L.par_piptrack_f32(par.dev, ptr(mag_t), c.frames, c.bins, c.pitch if c.pitch != c.bins else 0, float(c.scale), float(c.offset),
                                c.fft_size, c.sr, c.fmin, c.fmax, c.threshold, ptr(outs[0]), ptr(outs[1]), par.stream())
    assert rc == 0, (rc, par.lib.last_error())
    t.cuda.synchronize()
    assert np.array_equal(bits(mag_t.cpu().numpy()), bits(c.mag)), "the input (padding included) was written"
    res = []
    for o in outs:
        h = o.cpu().numpy()
        assert np.all(np.isnan(h[cells:])), "cells behind the output were written"
        assert not np.any(np.isnan(h[:cells])), "cells of the output were left unwritten"
        res.append(h[:cells].reshape(c.frames, c.bins))
    return res


pip_totals = {"cells": 0, "peaks": 0, "pitch_cells": 0, "mag_cells": 0, "pitch_ulp": 0, "mag_ulp": 0}


def compare_piptrack(name, got_p, got_m, want_p, want_m):
    dp, dm = bits(got_p) != bits(want_p), bits(got_m) != bits(want_m)
    pattern = int(np.sum((got_p != 0) != (want_p != 0)))
    up_, um_ = (int(ulps32(got_p, want_p)[dp].max()) if dp.any() else 0), (int(ulps32(got_m, want_m)[dm].max()) if dm.any() else 0)
    pip_totals["cells"] += want_p.size
    pip_totals["peaks"] += int(np.sum(want_p != 0))
    pip_totals["pitch_cells"] += int(dp.sum())
    pip_totals["mag_cells"] += int(dm.sum())
    pip_totals["pitch_ulp"] = max(pip_totals["pitch_ulp"], up_)
    pip_totals["mag_ulp"] = max(pip_totals["mag_ulp"], um_)
    print(f"\npiptrack {name}: {want_p.size} cells, {int(np.sum(want_p != 0))} peaks; differing pitches {int(dp.sum())} (max {up_} ulp), "
          f"magnitudes {int(dm.sum())} (max {um_} ulp), peak pattern {pattern}; so far {pip_totals}", end="")
    assert pattern == 0, (name, "peak pattern", np.argwhere((got_p != 0) != (want_p != 0))[:5].tolist())
    assert not dp.any(), (name, "pitches", np.argwhere(dp)[:5].tolist(), got_p[dp][:5], want_p[dp][:5])
    assert not dm.any(), (name, "magnitudes", np.argwhere(dm)[:5].tolist(), got_m[dm][:5], want_m[dm][:5])


@pytest.mark.parametrize("c", T.PIP_CASES, ids=[c.name for c in T.PIP_CASES])
def test_piptrack_equals_the_float32_statement_bit_for_bit(par, c):
    want_p, want_m = T.piptrack_statement(c)
    got_p, got_m = run_piptrack(par, c)
    compare_piptrack(c.name, got_p, got_m, want_p, want_m)


def test_piptrack_wrapper_with_defaults_equals_the_statement_bit_for_bit(par):
    """wow_detection.piptrack_dev on a get_mag spectrogram (1024 / 256, Hann, 101 frames of the pilot), default scale and offset,
    against the statement built from the same device magnitudes: what test_hip_parity.test_partials_tracker_piptrack asserts with
    tolerances, exactly."""
    import inputs
    from pyaudiorestoration_amd import fourier, wow_detection
    sr, n_fft, hop = 48000, 1024, 256
    x = inputs.pilot(100 * hop, sr)
    mag = fourier.get_mag(up(par, x), n_fft, hop, "hann", 1)                # (bins, frames) view of the frame-major buffer
    host = np.ascontiguousarray(mag.cpu().numpy().T)
    frames, bins = host.shape
    assert bins == n_fft // 2 + 1 and 95 <= frames <= 105 and host.dtype == np.float32
    for fmin, fmax, thr in ((150.0, 4000.0, 0.1), (3000.0, 5000.0, 0.15), (0.0, float(sr), 0.01)):
        c = T.PipCase("wrapper", host, bins, frames, bins, n_fft, float(sr), fmin, fmax, thr, np.float32(np.sqrt(n_fft)), np.float32(1e-7),
                      False)
        want_p, want_m = T.piptrack_statement(c)
        assert np.count_nonzero(want_p) > (frames if thr == 0.01 else 40)           # the pilot's line; with it the noise floor's peaks
        if thr == 0.1:
            p_t, m_t = wow_detection.piptrack_dev(mag, n_fft, sr, fmin, fmax)        # every default
        else:
            p_t, m_t = wow_detection.piptrack_dev(mag, n_fft, sr, fmin, fmax, thr)
        compare_piptrack(f"wrapper {fmin} {fmax} {thr}", p_t.cpu().numpy().T, m_t.cpu().numpy().T, want_p, want_m)


# ================================================================================================ correlation
corr_worst = {"integer": 0.0, "realistic": 0.0, "rows": 0.0}


def run_corr(par, c, pad):
    """-> (rc, R [(count + 1)][n], changes [count], freqs [count]); log_mean = 0 and log_span = n, so that freqs = exp2(cumsum)"""
    t = par.torch
    mag = T.pitched(c.mag, pad) if pad else c.mag
    mag_t, M_t, w_t = up(par, mag), up(par, c.M), up(par, c.wind)
    wl = int(par.L.par_track_corr_work_len(c.count, c.n))
    assert wl == (c.count + 1) * c.n + c.count
    work = t.full((wl + GUARD,), float("nan"), dtype=t.float64, device="cuda")
    freqs = t.full((c.count + GUARD,), float("nan"), dtype=t.float64, device="cuda")
    status = t.full((1,), 77, dtype=t.int32, device="cuda")
    rc = par.L.par_track_corr_f64(par.dev, ptr(mag_t), c.n_frames, c.bins, c.bins + pad if pad else 0, c.NL, c.NU, c.count, ptr(M_t), ptr(w_t),
                                  c.n, float(c.n), 0.0, ptr(work), ptr(freqs), ptr(status), par.stream())
    t.cuda.synchronize()
    assert np.array_equal(bits(mag_t.cpu().numpy()), bits(mag)), "the input (padding included) was written"
    w, f = work.cpu().numpy(), freqs.cpu().numpy()
    assert np.all(np.isnan(w[wl:])) and np.all(np.isnan(f[c.count:])), "cells behind work / freqs were written"
    return rc, w[:(c.count + 1) * c.n].reshape(c.count + 1, c.n), w[(c.count + 1) * c.n:wl], f[:c.count]


def compare_corr(c, st, changes, freqs, kind, tol):
    nan = np.isnan(st["changes"])
    assert np.array_equal(np.isnan(changes), nan), (c.name, changes, st["changes"])
    assert np.array_equal(np.isnan(freqs), np.isnan(st["cum"])), (c.name, freqs, st["cum"])
    ok = ~np.isnan(st["cum"])
    err_c = float(np.max(np.abs(changes[~nan] - st["changes"][~nan]), initial=0.0))
    err_f = float(np.max(np.abs(np.log2(freqs[ok]) - st["cum"][ok]), initial=0.0))
    corr_worst[kind] = max(corr_worst[kind], err_c, err_f)
    print(f"\ncorrelation {c.name}: |changes - statement| {err_c:.3e} lags, |log2 freqs - cumsum| {err_f:.3e} lags; worst so far {corr_worst}",
          end="")
    assert np.array_equal(np.rint(c.n // 2 - changes[~nan]), st["peaks"][~nan]), (c.name, "another lag", changes, st["peaks"])
    assert err_c <= tol and err_f <= tol, (c.name, err_c, err_f, tol)
    assert tol <= SAME_MAG_TOL


@pytest.mark.parametrize("c", T.CORR_CASES, ids=[c.name for c in T.CORR_CASES])
def test_correlation_integer_cases(par, c):
    want_R = T.corr_rows(c)
    last_lag = any(sp[0] == "last_lag" for sp in c.special.values())
    packed = run_corr(par, c, 0)
    pitched = run_corr(par, c, 37)
    for a, b in zip(packed, pitched):                       # pitched rows (3e38 in the padding) and packed rows: the same bits
        assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b))), c.name
    rc, R, changes, freqs = packed
    assert np.array_equal(bits(R), bits(want_R)), (c.name, np.argwhere(bits(R) != bits(want_R))[:5].tolist())
    if last_lag:
        assert rc == 6, (rc, par.lib.last_error())          # PAR_ERR_INDEX
        assert "par_track_corr_f64" in par.lib.last_error() and "last lag" in par.lib.last_error()
        with pytest.raises(IndexError):
            T.corr_statement(c)
        with pytest.raises(IndexError):
            par.lib.check(rc)
        return
    assert rc == 0, (rc, par.lib.last_error())
    st = T.corr_statement(c)
    compare_corr(c, st, changes, freqs, "integer", CORR_TOL_INTEGER)
    for i, sp in c.special.items():
        if sp[0] in ("tie", "tie_below_max"):
            assert int(np.rint(c.n // 2 - changes[i])) == sp[1] == st["peaks"][i], (c.name, changes[i], sp)
        elif sp[0] == "lag0":
            assert st["peaks"][i] == 0 and abs(changes[i] - c.n // 2) < 0.5


@pytest.mark.parametrize("c", T.CORR_REALISTIC, ids=[c.name for c in T.CORR_REALISTIC])
def test_correlation_realistic_cases(par, c):
    st = T.corr_statement(c)
    packed = run_corr(par, c, 0)
    pitched = run_corr(par, c, 37)
    for a, b in zip(packed, pitched):
        assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b))), c.name
    rc, R, changes, freqs = packed
    assert rc == 0, (rc, par.lib.last_error())
    err_R = float(np.max(np.abs(R - st["R"])) / np.max(np.abs(st["R"])))
    corr_worst["rows"] = max(corr_worst["rows"], err_R)
    print(f"\ncorrelation {c.name}: |R - statement| / max |R| {err_R:.3e}", end="")
    assert err_R <= CORR_TOL_ROWS <= SAME_MAG_TOL
    compare_corr(c, st, changes, freqs, "realistic", CORR_TOL_REALISTIC)


# ================================================================================================ zero crossings
def run_zc(par, x_t, n, idx_cap, work=None):
    """-> (rc, count, idx[idx_cap] or None (count-only form), work); idx starts as -1 with guard cells behind it"""
    t = par.torch
    wl = int(par.L.par_zero_crossings_work_len(n))
    if work is None:
        work = t.full((wl + GUARD,), -1, dtype=t.int64, device="cuda")
    idx = None if idx_cap is None else t.full((idx_cap + GUARD,), -1, dtype=t.int64, device="cuda")
    cnt = ctypes.c_int64(-5)
    rc = par.L.par_zero_crossings_f64(par.dev, ptr(x_t), n, ptr(work), None if idx is None else ptr(idx), 0 if idx is None else idx_cap,
                                      ctypes.byref(cnt), par.stream())
    t.cuda.synchronize()
    w = work.cpu().numpy()
    assert np.all(w[wl:] == -1), "cells behind work were written"
    return rc, cnt.value, None if idx is None else idx.cpu().numpy(), w[:wl]


@pytest.mark.parametrize("name", list(T.ZC_VECTORS))
def test_zero_crossings_on_special_values(par, name):
    x = T.ZC_VECTORS[name]
    want = T.zc_statement(x)
    x_t = up(par, x)
    rc, count, _, _ = run_zc(par, x_t, len(x), None)        # the count-only form
    assert rc == 0 and count == len(want), (rc, count, len(want), par.lib.last_error())
    rc, count, idx, _ = run_zc(par, x_t, len(x), len(want))
    assert rc == 0 and count == len(want)
    assert np.array_equal(idx[:count], want), (name, np.argwhere(idx[:count] != want)[:5].tolist())
    assert np.all(idx[count:] == -1), "cells behind idx were written"
    assert np.array_equal(bits(x_t.cpu().numpy()), bits(x))
    if len(want):                                           # one cell too few: reported, the count still returned, nothing written
        rc, count, idx, _ = run_zc(par, x_t, len(x), len(want) - 1)
        assert rc == 4 and count == len(want), (rc, count)                       # PAR_ERR_WORKSPACE
        assert "par_zero_crossings_f64" in par.lib.last_error() and np.all(idx == -1)


def test_zero_crossings_of_nothing_launch_nothing(par):
    x_t = up(par, T.ZC_SEQUENCE[4:6])                       # nan, 1.0: a crossing, were n 2
    for n in (0, 1):
        for cap in (None, 4):
            rc, count, idx, work = run_zc(par, x_t, n, cap)
            assert rc == 0 and count == 0 and np.all(work == -1) and (idx is None or np.all(idx == -1)), (n, cap, rc, count)
    rc, count, idx, _ = run_zc(par, x_t, 2, 4)
    assert rc == 0 and count == 1 and idx[0] == 0
