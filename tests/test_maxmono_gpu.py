"""GPU checks of MaxMono (dropouts_gui.MainWindow.process_max_mono): par_select_spectrum_f32 against numpy bit for bit, the fused
par_maxmono_stft_f32 against the composed statement (K_stft's spectra, numpy's selection on the host, K_istft) at every compiled
size, exact-relation signals that pin the tie rule, the Python layer against the reference's own results
(tests/golden/maxmono.npz, written by tools/gen_golden_maxmono.py) and the written files.

Every buffer a kernel reads or writes lies inside a larger tensor with guard cells on both sides (Guarded), strided outputs
have sentinels in the cells between.  tests/test_maxmono_cpu.py proves the preconditions of the inputs and the power of the
fused test.  pytest -s prints the measured figures (NOTES.md, MaxMono)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import maxmono_inputs as I
import maxmono_np as M
import renoiser_np
import stft_np as N
from test_heal_kernels_gpu import Guarded
from test_renoiser_gpu import FUSED_TOL, OUT_BLOCK, block_relerr, spectrum_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
GUARD = 64
NAN32 = np.float32(np.nan)


@pytest.fixture(scope="module")
def par():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pyaudiorestoration_amd import _dev, _lib

    class P:
        pass
    p = P()
    p.torch, p.dev, p.L, p.check, p.stream = torch, 0, _lib.lib(), _lib.check, lambda: _dev.stream_ptr(0)
    return p


# ------------------------------------------------------------------------------------------------ 1. the selection kernel
def run_select(par, c, pitch=0, want_min=True):
    """-> (max, min) as the kernel left them, padding and guards checked"""
    frames, bins = c.L.shape
    p = pitch or bins

    def pitched(a):
        whole = np.full((frames, p), I.SPEC_SENTINEL, dtype=np.complex64)
        whole[:, :bins] = a
        return whole
    gL, gR = Guarded(par, pitched(c.L), 2, I.SPEC_SENTINEL), Guarded(par, pitched(c.R), 2, I.SPEC_SENTINEL)
    blank = np.full((frames, p), I.SPEC_SENTINEL, dtype=np.complex64)
    gmax, gmin = Guarded(par, blank, 2, I.SPEC_SENTINEL), Guarded(par, blank, 2, I.SPEC_SENTINEL)
    rc = par.L.par_select_spectrum_f32(par.dev, gL.ptr(), gR.ptr(), frames, bins, pitch, gmax.ptr(), gmin.ptr() if want_min else None,
                                       par.stream())
    assert rc == OK, rc
    par.torch.cuda.synchronize()
    assert gL.unchanged() and gR.unchanged(), "an input was written"
    out = []
    for g, used in ((gmax, True), (gmin, want_min)):
        if not used:
            assert g.unchanged(), "the NULL output's neighbour was written"
            out.append(None)
            continue
        body = g.read()
        assert g.guards_intact()
        assert np.array_equal(I.bits(body[:, bins:]), I.bits(blank[:, bins:])), "padding cells were written"
        out.append(body[:, :bins])
    return out


def assert_selected(got, c, label):
    want = M.select(c.L, c.R)
    for g, w, op in zip(got, want, ("max", "min")):
        if g is None:
            continue
        same = I.bits(g) == I.bits(w)
        assert same.all(), (label, op, int((~same).sum()), np.argwhere(~same)[:5])


def test_select_ties_and_their_neighbours_bit_for_bit(par):
    c = I.tie_spectra()
    got = run_select(par, c)
    assert_selected(got, c, "ties")
    tie = c.cls == 0
    assert np.array_equal(I.bits(got[0])[tie], I.bits(c.R)[tie]) and np.array_equal(I.bits(got[1])[tie], I.bits(c.R)[tie])
    assert np.array_equal(I.bits(got[0])[0], I.bits(c.R)[0])                   # the all-tie row
    print(f"\nselect: {int(tie.sum())} ties -> R in both outputs; {int((c.cls == 1).sum())} ulp-under, {int((c.cls == 2).sum())} ulp-over, bit-identical")


@pytest.mark.parametrize("pitch", (0, 264))
def test_select_two_pitches_leave_the_padding(par, pitch):
    c = I.free_spectra(37, 257, 5)
    got = run_select(par, c, pitch)
    assert_selected(got, c, ("pitch", pitch))
    share = float(np.mean(I.bits(got[0]) == I.bits(c.L)))
    assert 0.4 < share < 0.6, share


def test_select_second_pass_of_the_frame_loop(par):
    c = I.free_spectra(I.SELECT_GRID_ROWS + 5, 33, 6)
    got = run_select(par, c)
    assert_selected(got, c, "second pass")
    tail = slice(I.SELECT_GRID_ROWS, None)
    assert (I.bits(got[0])[tail] == I.bits(c.L)[tail]).any() and (I.bits(got[0])[tail] == I.bits(c.R)[tail]).any()


def test_select_special_values_copy_bits(par):
    c = I.special_spectra()
    got = run_select(par, c)
    assert_selected(got, c, "special")                                       # NaN cells included: the selection copies bits


def test_select_without_the_min_output(par):
    c = I.free_spectra(9, 300, 7)
    got = run_select(par, c, want_min=False)
    assert got[1] is None
    assert_selected(got, c, "max only")


def test_select_argument_errors(par):
    t = par.torch
    a = t.zeros((4, 8), dtype=t.complex64, device="cuda")
    b, o1, o2 = t.zeros_like(a), t.zeros_like(a), t.zeros_like(a)
    P = lambda x: ctypes.c_void_p(x.data_ptr())
    f = par.L.par_select_spectrum_f32
    s = par.stream()
    assert f(par.dev, None, P(b), 4, 8, 0, P(o1), P(o2), s) == ERR_ARG
    assert f(par.dev, P(a), None, 4, 8, 0, P(o1), P(o2), s) == ERR_ARG
    assert f(par.dev, P(a), P(b), 4, 8, 0, None, None, s) == ERR_ARG
    assert f(par.dev, P(a), P(b), -1, 8, 0, P(o1), P(o2), s) == ERR_ARG
    assert f(par.dev, P(a), P(b), 4, 0, 0, P(o1), P(o2), s) == ERR_ARG
    assert f(par.dev, P(a), P(b), 4, 8, 7, P(o1), P(o2), s) == ERR_ARG          # pitch < bins
    assert f(par.dev, P(a), P(b), 4, 8, 0, P(a), P(o2), s) == ERR_ARG           # an output on an input
    assert f(par.dev, P(a), P(b), 4, 8, 0, P(o1), P(b), s) == ERR_ARG
    assert f(par.dev, P(a), P(b), 4, 8, 0, P(o1), P(o1), s) == ERR_ARG          # the outputs on each other
    assert f(par.dev, P(a), P(b), 4, 8, 0, P(o1), ctypes.c_void_p(o1.data_ptr() + 8), s) == ERR_ARG
    assert f(par.dev, P(a), P(b), 0, 8, 0, P(o1), P(o2), s) == OK               # no frames: nothing to do
    par.torch.cuda.synchronize()
    assert not bool(o1.abs().sum()) and not bool(o2.abs().sum())


# ------------------------------------------------------------------------------------------------ 2. the fused kernel
def window_t(par, n_fft):
    from pyaudiorestoration_amd import fourier
    return fourier.window_dev("blackmanharris", n_fft, par.dev)


def run_fused(par, x2, cl, cr, n_fft, hop, layout="split", want_min=True, expect=OK):
    """par_maxmono_stft_f32 on channels cl / cr of the interleaved x2 between NaN guards.  layout "split": y_max with stride 3
    among sentinels, y_min packed; "columns": the two columns of one (n, 2) buffer; -> (y_max, y_min)"""
    n, ch = x2.shape
    gx = Guarded(par, x2, GUARD, NAN32)
    w = window_t(par, n_fft)
    if layout == "split":
        ga = Guarded(par, np.full((n, 3), I.SENTINEL, np.float32), GUARD, I.SENTINEL)
        gb = Guarded(par, np.full((n,), I.SENTINEL, np.float32), GUARD, I.SENTINEL)
        pa, sa, pb, sb = ga.ptr(), 3, gb.ptr(), 1
    else:
        ga = gb = Guarded(par, np.full((n, 2), I.SENTINEL, np.float32), GUARD, I.SENTINEL)
        pa, sa, pb, sb = ga.ptr(), 2, ga.ptr(1), 2
    rc = par.L.par_maxmono_stft_f32(par.dev, gx.ptr(cl), gx.ptr(cr), n, ch, n_fft, hop, ctypes.c_void_p(w.data_ptr()), pa, sa,
                                    pb if want_min else None, sb, par.stream())
    assert rc == expect, (rc, expect)
    par.torch.cuda.synchronize()
    assert gx.unchanged(), "the input was written"
    if expect != OK:
        assert ga.unchanged() and gb.unchanged(), "an output was written by a refused call"
        return None, None
    a = ga.read()
    assert ga.guards_intact()
    if layout == "split":
        assert np.all(a[:, 1:] == I.SENTINEL), "cells between the strided outputs were written"
        y_max = a[:, 0].copy()
        if want_min:
            y_min = gb.read().copy()
            assert gb.guards_intact()
        else:
            assert gb.unchanged()
            y_min = None
    else:
        y_max = a[:, 0].copy()
        if want_min:
            y_min = a[:, 1].copy()
        else:
            assert np.all(a[:, 1] == I.SENTINEL), "the NULL output's column was written"
            y_min = None
    for y in (y_max, y_min):
        assert y is None or not np.any(y == I.SENTINEL), "samples not written"
    return y_max, y_min


def istft_of(par, S, n_fft, hop, n):
    """K_istft (length n) of a host spectrogram (frames, bins) complex64"""
    from pyaudiorestoration_amd import _dev, fourier
    fm = _dev.to_dev(np.ascontiguousarray(S, dtype=np.complex64), par.torch.complex64, par.dev)
    return _dev.to_host(fourier.istft_dev(fm.T, hop, window_t(par, n_fft), length=n, dev=par.dev))


_composed = {}


def composed(par, x2, cl, cr, n_fft, hop, key):
    """The composed statement, computed once per input: K_stft's two spectra downloaded, selected by numpy, uploaded, K_istft.
    -> dict(SL, SR, y_max, y_min, y_L, y_R); never written to"""
    key = (key, cl, cr, n_fft, hop)
    if key not in _composed:
        from pyaudiorestoration_amd import _dev
        n = len(x2)
        SL = _dev.to_host(spectrum_dev(np.ascontiguousarray(x2[:, cl]), n_fft, hop, par.dev)).copy()
        SR = _dev.to_host(spectrum_dev(np.ascontiguousarray(x2[:, cr]), n_fft, hop, par.dev)).copy()
        d_max, d_min = M.select(SL, SR)
        r = dict(SL=SL, SR=SR, y_max=istft_of(par, d_max, n_fft, hop, n), y_min=istft_of(par, d_min, n_fft, hop, n))
        for v in r.values():
            v.setflags(write=False)
        _composed[key] = r
    return _composed[key]


def rel_err(got, want):
    peak = max(float(np.max(np.abs(want))), 1e-30)
    return float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)))) / peak


def fused_err(got, ref, op, n_fft, hop):
    """largest difference from the composed statement, of its peak, over the samples no near-tie bin reaches (the header's
    contract: such a bin may hold either channel).  So that the excusal cannot empty the test: near-tie bins are at most 1e-4
    of the bins (test 4's share; one bin where that is less than one), every case compares some samples, and a case of 25
    transforms or more -- where one frame's reach is 4 % -- compares at least 3/4 of them.  tests/test_maxmono_cpu.py shows that
    independent spectra hold fewer than 5e-5 such bins."""
    want = ref[f"y_{op}"]
    n = len(want)
    near = M.near_ties(ref["SL"], ref["SR"])
    assert near.sum() <= max(1, 1e-4 * near.size), (n_fft, hop, n, int(near.sum()), near.size)
    ok = M.unreached(near, hop, n_fft, n)
    assert ok.any() and (n < 25 * n_fft or ok.sum() >= 0.75 * n), (n_fft, hop, n, int(ok.sum()))
    peak = max(float(np.max(np.abs(want))), 1e-30)
    return float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))[ok])) / peak


@pytest.mark.parametrize("n_fft,hop", I.FUSED_SIZES)
def test_fused_equals_composed(par, n_fft, hop):
    worst = 0.0
    for n in I.lengths(n_fft, hop):
        x2 = I.stereo(n, n_fft + hop)
        ref = composed(par, x2, 0, 1, n_fft, hop, ("stereo", n))
        y_max, y_min = run_fused(par, x2, 0, 1, n_fft, hop)
        assert y_max.shape == y_min.shape == (n,) and np.isfinite(y_max).all() and np.isfinite(y_min).all()
        e = max(fused_err(y_max, ref, "max", n_fft, hop), fused_err(y_min, ref, "min", n_fft, hop))
        worst = max(worst, e)
        assert e <= FUSED_TOL, (n_fft, hop, n, e)
        again = run_fused(par, x2, 0, 1, n_fft, hop)
        assert np.array_equal(I.bits(again[0]), I.bits(y_max)) and np.array_equal(I.bits(again[1]), I.bits(y_min)), "two runs differ"
    print(f"\nfused vs composed {n_fft}/{hop}: lengths {I.lengths(n_fft, hop)}, largest difference {worst:.3e} of the peak", end="")


@pytest.mark.parametrize("n_fft,hop", ((64, 16), (512, 96), (2048, 512), (8192, 2048)))
def test_fused_layouts_channel_order_and_null_output(par, n_fft, hop):
    n = I.lengths(n_fft, hop)[-1]
    x2 = I.stereo(n, n_fft + hop)
    # channel 1 as L and channel 0 as R: the tie rule makes the order matter, the composed statement is taken in that order
    ref = composed(par, x2, 1, 0, n_fft, hop, ("stereo", n))
    y_max, y_min = run_fused(par, x2, 1, 0, n_fft, hop, layout="columns")
    assert fused_err(y_max, ref, "max", n_fft, hop) <= FUSED_TOL and fused_err(y_min, ref, "min", n_fft, hop) <= FUSED_TOL
    split = run_fused(par, x2, 1, 0, n_fft, hop, layout="split")
    assert np.array_equal(I.bits(split[0]), I.bits(y_max)) and np.array_equal(I.bits(split[1]), I.bits(y_min)), "the layout changed the result"
    for layout in ("split", "columns"):
        only, none = run_fused(par, x2, 1, 0, n_fft, hop, layout=layout, want_min=False)
        assert none is None and np.array_equal(I.bits(only), I.bits(y_max)), "y_min == NULL changed y_max"
    # three channels in the file: strides and views are the caller's
    x3 = np.concatenate([x2, np.full((n, 1), NAN32, np.float32)], axis=1)
    y3 = run_fused(par, x3, 1, 0, n_fft, hop)
    assert np.array_equal(I.bits(y3[0]), I.bits(y_max)) and np.array_equal(I.bits(y3[1]), I.bits(y_min))


def test_fused_limits_and_argument_errors(par):
    big, first = I.largest_fused_hop(8192), I.largest_fused_hop(8192) + 1
    assert par.L.par_maxmono_stft_supported(8192, big) == 1 and par.L.par_maxmono_stft_supported(8192, first) == 0
    x2 = I.stereo(3000, 1)
    for n_fft, hop in ((8192, first), (8192, 8192), (16384, 4096), (8, 2), (1000, 250), (512, 513)):
        assert par.L.par_maxmono_stft_supported(n_fft, hop) == 0
        run_fused(par, x2, 0, 1, n_fft, hop, expect=ERR_UNSUPPORTED)
        run_fused(par, x2, 0, 1, n_fft, hop, layout="columns", expect=ERR_UNSUPPORTED)
    for n_fft, hop in I.FUSED_SIZES:
        assert par.L.par_maxmono_stft_supported(n_fft, hop) == 1
        assert par.L.par_maxmono_stft_transformed_frames(100000, n_fft, hop) >= -(-100000 // hop)
    assert par.L.par_maxmono_stft_transformed_frames(100000, 8192, first) == 0
    run_fused(par, x2, 0, 1, 512, 0, expect=ERR_ARG)
    t = par.torch
    x = t.zeros(4096, device="cuda")
    y = t.full((4096,), float(I.SENTINEL), device="cuda")
    w = window_t(par, 512)
    P = lambda v: ctypes.c_void_p(v.data_ptr())
    f = par.L.par_maxmono_stft_f32
    s = par.stream()
    assert f(par.dev, None, P(x), 1000, 1, 512, 128, P(w), P(y), 1, P(y[2000:]), 1, s) == ERR_ARG
    assert f(par.dev, P(x), None, 1000, 1, 512, 128, P(w), P(y), 1, P(y[2000:]), 1, s) == ERR_ARG
    assert f(par.dev, P(x), P(x), 1000, 1, 512, 128, None, P(y), 1, P(y[2000:]), 1, s) == ERR_ARG
    assert f(par.dev, P(x), P(x), 1000, 1, 512, 128, P(w), None, 1, None, 1, s) == ERR_ARG
    assert f(par.dev, P(x), P(x), 0, 1, 512, 128, P(w), P(y), 1, P(y[2000:]), 1, s) == ERR_ARG
    assert f(par.dev, P(x), P(x), 1000, 0, 512, 128, P(w), P(y), 1, P(y[2000:]), 1, s) == ERR_ARG
    assert f(par.dev, P(x), P(x), 1000, 1, 512, 128, P(w), P(y), 0, P(y[2000:]), 1, s) == ERR_ARG
    assert f(par.dev, P(x), P(x), 1000, 1, 512, 128, P(w), P(y), 1, P(y[2000:]), 0, s) == ERR_ARG
    t.cuda.synchronize()
    assert bool((y == float(I.SENTINEL)).all())


# ------------------------------------------------------------------------------------------------ 3. exact relations
@pytest.mark.parametrize("n_fft,hop", ((16, 4), (256, 64), (2048, 512), (8192, 1024)))
def test_exact_relations_pin_the_tie_rule(par, n_fft, hop):
    """R = -L (and L = -R): negation is exact through the whole forward path, every bin ties, both outputs are the ISTFT of D_R
    -- a >= in place of > returns the sign-flipped signal, 2 x the peak away.  R = 2 L: max <- R, min <- L in every bin;
    R = L / 2: the reverse.  No oracle: K_stft / K_istft of the single channels are the statement."""
    from pyaudiorestoration_amd import _dev
    n = I.lengths(n_fft, hop)[-1]
    a = I.stereo(n, 3)[:, 0].copy()

    def through(x):                                                     # K_istft(K_stft(fix_length(x))) of one channel
        return istft_of(par, _dev.to_host(spectrum_dev(x, n_fft, hop, par.dev)), n_fft, hop, n)
    for name, L, R, want_max, want_min in (("R = -L", a, -a, "R", "R"), ("L = -R", -a, a, "R", "R"),
                                           ("R = 2 L", a, 2 * a, "R", "L"), ("R = L / 2", a, a / 2, "L", "R")):
        x2 = np.ascontiguousarray(np.stack([L, R], axis=1).astype(np.float32))
        assert np.array_equal(x2[:, 0], L) and np.array_equal(x2[:, 1], R)
        y_max, y_min = run_fused(par, x2, 0, 1, n_fft, hop, layout="columns")
        side = {"L": through(x2[:, 0].copy()), "R": through(x2[:, 1].copy())}
        e_max, e_min = rel_err(y_max, side[want_max]), rel_err(y_min, side[want_min])
        print(f"\n{n_fft}/{hop} {name}: max {e_max:.2e}, min {e_min:.2e} of the peak", end="")
        assert e_max <= FUSED_TOL and e_min <= FUSED_TOL, (n_fft, hop, name, e_max, e_min)
        other = {"L": "R", "R": "L"}
        assert rel_err(y_max, side[other[want_max]]) > 0.1                   # the other choice is far away


# ------------------------------------------------------------------------------------------------ 4. the reference's results
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "maxmono.npz"))


@pytest.fixture(scope="module")
def fixture_stereo(gold):
    from pyaudiorestoration_amd import io_ops
    sig, sr, _ = io_ops.read_file(os.path.join(GOLDEN, "nr_signal.wav"))
    sig = sig if sig.ndim == 2 else sig[:, None]
    return np.concatenate([sig, np.roll(sig, int(gold["stereo_shift"]), axis=0)], axis=1).astype(np.float32), sr


@pytest.mark.parametrize("setting", (0, 1, 2))
def test_against_the_reference_fixture(par, gold, fixture_stereo, setting):
    """Our decisions (numpy's np.abs comparison on K_stft's spectra, which the kernels take bit for bit: tests above) against the
    reference's float64 decisions.  A disagreement is excused only where the float64 magnitudes of the two channels differ by no
    more than the sum of the two frames' transform bounds; the outputs are compared in the 1024-sample blocks no disagreeing
    bin reaches.  Measured on the MI355X: see NOTES.md, MaxMono."""
    from pyaudiorestoration_amd import _dev, dropouts
    signal, sr = fixture_stereo
    n = len(signal)
    fft, hop = (int(v) for v in gold["settings"][setting])
    k = f"{fft}_{hop}"
    stride, frames, bins = int(gold["stride"]), int(gold[f"{k}_frames"]), fft // 2 + 1
    assert str(gold["spec_dtype"]) == "complex128"
    SL = _dev.to_host(spectrum_dev(signal[:, 0].copy(), fft, hop, par.dev))
    SR = _dev.to_host(spectrum_dev(signal[:, 1].copy(), fft, hop, par.dev))
    assert SL.shape == (frames, bins)
    ours = dict(zip(("max", "min"), M.masks(SL, SR)))
    # float64 magnitudes of the same float32 frames and K_stft's bound per frame, of the frame's largest bin
    w = N.window32("blackmanharris", fft)
    pad = np.zeros((n + fft // 2, 2), np.float32)
    pad[:n] = signal
    mL, mR = N.mag64(N.stft64(pad[:, 0], fft, hop, 1, w)), N.mag64(N.stft64(pad[:, 1], fft, hop, 1, w))
    b = N.bound(N.R_REG, fft)
    slack = b * (mL.max(axis=1) + mR.max(axis=1))[:, None]
    near = np.abs(mL - mR) <= slack
    block = 1024
    results = {}
    for fused in (True, False):
        y = dropouts.max_mono(signal, sr, fft, hop, fused=fused)
        for op, yy in zip(("max", "min"), y):
            assert yy.shape == (n,) and yy.dtype == np.float32 and np.isfinite(yy).all()
            ref = M.unpack_mask(gold[f"{k}_mask_{op}"], frames, bins)
            dis = ours[op] != ref
            bad = dis & ~near
            assert not bad.any(), (k, op, np.argwhere(bad)[:5])
            assert dis.sum() <= 1e-4 * dis.size, (k, op, int(dis.sum()))
            ok = np.ones(-(-n // block), bool)
            for lo, hi in renoiser_np.reach(np.argwhere(dis)[:, 0], hop, fft, n):
                ok[lo // block:(hi - 1) // block + 1] = False
            assert ok.sum() >= 0.75 * len(ok), (k, op, int(ok.sum()), len(ok))
            # strided samples: block i of block // stride stored samples lies in block i of the file
            err = block_relerr(yy[::stride], gold[f"{k}_y_{op}"], block // stride, blocks=ok)
            results[(fused, op)] = (int(dis.sum()), int(ok.sum()), len(ok), err)
            assert err <= OUT_BLOCK, (k, op, fused, err)
    for (fused, op), (d, c, t, err) in results.items():
        print(f"\n{k} {'fused' if fused else 'composed'} {op}: {d} of {frames * bins} bins disagree ({int(near.sum())} within the transform "
              f"bounds), {c} of {t} blocks compared, output {err:.2e} of the block peak", end="")


# ------------------------------------------------------------------------------------------------ 5. files
def test_process_and_cli_write_the_same_bytes(par, gold, fixture_stereo, tmp_path):
    from pyaudiorestoration_amd import dropouts, io_ops
    signal, sr = fixture_stereo
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    for d in (a, b):
        io_ops.write_wav_float(str(d / "tape.wav"), signal, sr)
    paths = dropouts.process(str(a / "tape.wav"), 2048, 4, device=par.dev)
    assert [os.path.basename(p) for p in paths] == ["tapemax.wav", "tapemin.wav"] and all(os.path.exists(p) for p in paths)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "pyaudiorestoration_amd.cli", "maxmono", "--fft", "2048", "--overlap", "4", str(b / "tape.wav")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for p, op in zip(paths, ("max", "min")):
        other = b / os.path.basename(p)
        assert open(p, "rb").read() == open(other, "rb").read()
        y, rate, ch = io_ops.read_file(p)
        y = y if y.ndim == 1 else y[:, 0]
        assert (rate, ch, len(y)) == (sr, 1, len(signal))
        assert block_relerr(y[::int(gold["stride"])], gold[f"2048_512_y_{op}"]) <= OUT_BLOCK * 10     # the near bins' blocks included
    mono = tmp_path / "mono.wav"
    io_ops.write_wav_float(str(mono), signal[:, 0], sr)
    with pytest.raises(ValueError, match="stereo"):
        dropouts.process(str(mono), device=par.dev)
    assert not os.path.exists(tmp_path / "monomax.wav")
