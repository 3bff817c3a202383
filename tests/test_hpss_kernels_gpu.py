"""par_hpss_f32 and par_residual_f32 (csrc/hpss.hip, ABI 109) at the C ABI, cell by cell, on the value classes of
tests/hpss_inputs.py (their properties are proved on the CPU in tests/test_hpss_inputs_cpu.py).  Every buffer lies between 64 guard
elements of a sentinel bit pattern, every launch is at most 130 x 130 cells.

  medians   bit for bit against hpss_np.median_reflect (np.sort of the reflected window at rank k // 2; np.sort puts NaN last, which
            is the kernel's rule: a NaN magnitude ranks above inf), any axis length from 1, so every fill of the last 64-wide tile
            and of the last run of four, and reflections that wrap many times.  NaN cells are compared by isnan.
  masks     on the pair table (every branch edge of softmask as a (harm, perc) pair).  Powers 2, inf, 1 and 0.5 equal
            hpss_np.mask bit for bit, NaN for NaN.  The general powers go through powf; they are compared with the float64 statement
            hpss_np.mask64.  Exactly one of the two powered ratios is 1, so one powf error passes through one rounded sum and one
            rounded quotient.  No accuracy figure for powf is stated in the documentation or the headers that ship with ROCm (the
            only figures there are OpenCL's, for other functions), so the project's MASK_ULP = 6 holds (tests/test_hpss_gpu.py);
            the measured worst per power is printed beside E_np, numpy's own distance from the float64 statement.
  products  equal numpy's `spec * mask` of the kernel's own masks bit for bit, NaN for NaN.  For complex64 that is numpy's
            complex product with mask + 0i (test_hpss_inputs_cpu.product_np states it part by part): an infinite or NaN part
            reaches both parts of the result.
  writes    pitch padding, guards and the input keep their bits; PAR_HPSS_HARMONIC leaves out_p alone; n_frames == 0 writes
            nothing; a second launch gives the same bits."""
import numpy as np
import pytest

import hpss_inputs as I
import hpss_np
from test_heal_kernels_gpu import Guarded, bits
from test_hpss_gpu import MASK_ULP

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL_BITS = 0xDEADBEEF                                              # -6.26e18 as a float32: no NaN, so guards compare as values too
SENTINEL = np.array([SENTINEL_BITS], np.uint32).view(np.float32)[0]
SENTINEL_C = np.complex64(complex(SENTINEL, SENTINEL))
COMPONENTS, MASKS, HARMONIC, MEDIANS = 0, 1, 2, 3


@pytest.fixture(scope="module")
def par():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pyaudiorestoration_amd import _dev, _lib

    class P:
        pass
    p = P()
    p.torch, p.dev, p.L, p.check, p.stream = torch, 0, _lib.lib(), _lib.check, lambda: _dev.stream_ptr(0)
    assert (_lib.HPSS_COMPONENTS, _lib.HPSS_MASKS, _lib.HPSS_HARMONIC, _lib.HPSS_MEDIANS) == (COMPONENTS, MASKS, HARMONIC, MEDIANS)
    return p


def sentinel_of(dtype):
    return SENTINEL_C if np.dtype(dtype) == np.complex64 else SENTINEL


def pitched(a, pitch):
    """(frames, bins) -> flat frames * pitch elements, the padding cells hold the sentinel"""
    out = np.full((a.shape[0], pitch), sentinel_of(a.dtype), dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out.reshape(-1)


class Launch:
    """one spectrogram and two outputs between guards; run() launches, checks everything outside the cells and returns them"""

    def __init__(self, par, spec, out_dtype, pitch=None):
        self.par, self.spec_np = par, spec
        self.frames, self.bins = spec.shape
        self.pitch = self.bins if pitch is None else pitch
        self.spec = Guarded(par, pitched(spec, self.pitch), GUARD, sentinel_of(spec.dtype))
        n = self.frames * self.pitch
        self.out = [Guarded(par, np.full(n, sentinel_of(out_dtype), dtype=out_dtype), GUARD, sentinel_of(out_dtype)) for _ in range(2)]

    def run(self, kind, kernel, power=2.0, margin=(1.0, 1.0), out_p=True, n_frames=None, explicit_pitch=True):
        p = self.par
        pitch = self.pitch if explicit_pitch else 0
        rc = p.L.par_hpss_f32(p.dev, self.spec.ptr(), int(np.iscomplexobj(self.spec_np)), self.frames if n_frames is None else n_frames, self.bins,
                              pitch, kernel[0], kernel[1], float(power), float(margin[0]), float(margin[1]), self.out[0].ptr(),
                              self.out[1].ptr() if out_p else None, kind, p.stream())
        p.check(rc)
        p.torch.cuda.synchronize()
        got = []
        for o in self.out:
            body = o.read().reshape(self.frames, self.pitch)
            assert o.guards_intact()
            assert (bits(body[:, self.bins:]) == SENTINEL_BITS).all()                       # the pitch padding
            got.append(np.ascontiguousarray(body[:, :self.bins]))
        assert self.spec.unchanged()
        return got

    def untouched(self, which):
        return self.out[which].unchanged()


def same(got, want):
    """bit for bit, NaN for NaN (per float32 part)"""
    g, w = np.ascontiguousarray(got).view(np.float32), np.ascontiguousarray(want).view(np.float32)
    if g.shape != w.shape:
        return False
    nan = np.isnan(w)
    return bool(np.array_equal(np.isnan(g), nan) and np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan]))


def where_differs(got, want):
    g, w = np.ascontiguousarray(got).view(np.float32), np.ascontiguousarray(want).view(np.float32)
    d = (np.isnan(g) != np.isnan(w)) | ((g.view(np.uint32) != w.view(np.uint32)) & ~np.isnan(w))
    at = np.argwhere(d)
    return int(d.sum()), [(tuple(int(v) for v in i), float(g[tuple(i)]), float(w[tuple(i)])) for i in at[:4]]


_MEDIANS = {}


def want_medians(key, mag, kernel):
    """the oracle, computed once per (array, size, axis)"""
    out = []
    for k, axis in ((kernel[0], 0), (kernel[1], 1)):
        if (key, k, axis) not in _MEDIANS:
            _MEDIANS[key, k, axis] = hpss_np.median_reflect(mag, k, axis)
        out.append(_MEDIANS[key, k, axis])
    return out


def check_medians(par, cls, shape, is_complex, seed=109):
    spec = I.make(cls, shape, seed, is_complex)
    mag = I.magnitudes(spec)
    run = Launch(par, spec, np.float32)
    for kernel in I.KERNEL_PAIRS:
        got = run.run(MEDIANS, kernel, explicit_pitch=False)
        want = want_medians((cls, shape, is_complex, seed), mag, kernel)
        for g, w, name in zip(got, want, ("harm", "perc")):
            assert g.dtype == np.float32 and same(g, w), (cls, shape, is_complex, kernel, name) + where_differs(g, w)


SWEEP_SHAPES = [(I.SWEEP_FRAMES, n) for n in I.AXIS_LENGTHS] + [(n, I.SWEEP_BINS) for n in I.AXIS_LENGTHS] + list(I.CORNER_SHAPES)


@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_medians_at_every_axis_length(par, shape):
    for is_complex in (False, True):
        check_medians(par, "uniform", shape, is_complex)


@pytest.mark.parametrize("cls,is_complex", [(c, False) for c in I.REAL_CLASSES[1:]] + [(c, True) for c in I.COMPLEX_CLASSES[1:]],
                         ids=lambda v: str(v))
def test_medians_of_the_value_classes(par, cls, is_complex):
    for shape in I.CLASS_SHAPES:
        check_medians(par, cls, shape, is_complex)


# ------------------------------------------------------------------------------------------------------------ pitch, guards
@pytest.mark.parametrize("shape", [(67, 66), (130, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", [MEDIANS, COMPONENTS])
def test_pitch_padding_guards_and_a_second_launch(par, shape, kind):
    bins = shape[1]
    spec = I.make("nan", shape, 7, True)
    out_dtype = np.float32 if kind == MEDIANS else np.complex64
    kernel = (31, 17)
    plain = Launch(par, spec, out_dtype).run(kind, kernel, 2.0, (2.0, 3.0))
    for pitch in (bins + 1, bins + 31, -(-(bins + 1) // 32) * 32):
        run = Launch(par, spec, out_dtype, pitch)
        first = run.run(kind, kernel, 2.0, (2.0, 3.0))
        for g, w in zip(first, plain):
            assert same(g, w) and np.isnan(w.view(np.float32)).any(), (shape, kind, pitch)
        again = run.run(kind, kernel, 2.0, (2.0, 3.0))                                      # into the same buffers
        for g, w in zip(again, first):
            assert np.array_equal(bits(g), bits(w)), (shape, kind, pitch)
    if kind == MEDIANS:
        want = want_medians(("nan", shape, True, 7), I.magnitudes(spec), kernel)
        assert same(plain[0], want[0]) and same(plain[1], want[1])


@pytest.mark.parametrize("kind", [COMPONENTS, MASKS, HARMONIC, MEDIANS])
def test_no_frames_writes_nothing(par, kind):
    spec = I.make("uniform", (5, 66), 8, True)
    run = Launch(par, spec, np.complex64, 70)
    got = run.run(kind, (3, 3), n_frames=0)
    assert run.untouched(0) and run.untouched(1)
    assert all((bits(g) == SENTINEL_BITS).all() for g in got)


# ------------------------------------------------------------------------------------------------------------------- masks
@pytest.fixture(scope="module")
def pair_tables():
    pairs = I.mask_pairs()
    return {t: (I.pair_table(pairs, t), (1, 3) if t else (3, 1), I.pair_table_expected(pairs, t)) for t in (False, True)}


def want_masks(harm, perc, power, margin, fn):
    one = margin == (1.0, 1.0)
    with np.errstate(all="ignore"):
        mh = fn(harm, perc * np.float32(margin[0]), power, one)
        mp = fn(perc, harm * np.float32(margin[1]), power, one)
    return [np.asarray(m, np.float32) for m in (mh, mp)]


@pytest.mark.parametrize("transposed", [False, True], ids=["frames", "bins"])
def test_pair_table_medians(par, pair_tables, transposed):
    table, kernel, (harm, perc) = pair_tables[transposed]
    got = Launch(par, table, np.float32).run(MEDIANS, kernel)
    assert same(got[0], harm) and same(got[1], perc), where_differs(got[0], harm) + where_differs(got[1], perc)


@pytest.mark.parametrize("transposed", [False, True], ids=["frames", "bins"])
@pytest.mark.parametrize("power", I.POWERS_EXACT, ids=str)
def test_masks_of_the_exact_powers_equal_numpy(par, pair_tables, transposed, power):
    table, kernel, (harm, perc) = pair_tables[transposed]
    run = Launch(par, table, np.float32)
    for margin in I.MARGINS:
        got = run.run(MASKS, kernel, power, margin)
        want = want_masks(harm, perc, power, margin, hpss_np.mask)
        for g, w, name in zip(got, want, ("mask_h", "mask_p")):
            assert same(g, w), (power, margin, name) + where_differs(g, w)
        nan_in = np.isnan(harm) | np.isnan(perc)
        if np.isfinite(power):
            assert np.isnan(got[0][nan_in]).all() and np.isnan(got[1][nan_in]).all() and nan_in.sum() >= 6 * 22
        else:
            assert not got[0][nan_in].any() and not got[1][nan_in].any()


@pytest.mark.parametrize("transposed", [False, True], ids=["frames", "bins"])
@pytest.mark.parametrize("power", I.POWERS_GENERAL, ids=str)
def test_masks_of_the_general_powers_against_float64(par, pair_tables, transposed, power):
    table, kernel, (harm, perc) = pair_tables[transposed]
    run = Launch(par, table, np.float32)
    worst, e_np = 0, 0
    for margin in I.MARGINS:
        got = run.run(MASKS, kernel, power, margin)
        want = want_masks(harm, perc, power, margin, hpss_np.mask64)
        numpys = want_masks(harm, perc, power, margin, hpss_np.mask)
        for g, w, n32 in zip(got, want, numpys):
            same_nan, d = hpss_np.ulp_distance_nan(g, w)
            worst, e_np = max(worst, d), max(e_np, hpss_np.ulp_distance_nan(n32, w)[1])
            print(f"\npower {power}, margin {margin}, {'bins' if transposed else 'frames'}: kernel {d} ulp from the float64 mask")
            assert same_nan, (power, margin) + where_differs(g, w)
            assert d <= MASK_ULP, (power, margin, d)
    print(f"\npower {power}: worst {worst} float32 ulp from the float64 mask (numpy's float32 mask: E_np = {e_np}); bound {MASK_ULP}")


# ---------------------------------------------------------------------------------------------------------------- products
def product_cases():
    return [("nan", True), ("wide", True), ("ties", True), ("signed", False), ("nan", False)]


@pytest.mark.parametrize("cls,is_complex", product_cases(), ids=lambda v: str(v))
@pytest.mark.parametrize("kind", [COMPONENTS, HARMONIC])
def test_products_equal_numpys_spec_times_the_kernels_masks(par, cls, is_complex, kind):
    shape, kernel = (67, 66), (5, 4)
    spec = I.make(cls, shape, 12, is_complex)
    for power, margin in ((2.0, (1.0, 1.0)), (np.inf, (1.0, 1.0)), (1.0, (2.0, 3.0))):
        masks = Launch(par, spec, np.float32).run(MASKS, kernel, power, margin)
        assert all(m.dtype == np.float32 for m in masks)
        with np.errstate(all="ignore"):
            want = [spec * m for m in masks]                                                # numpy's own product
        assert want[0].dtype == spec.dtype
        if cls in ("wide", "signed") and np.isinf(power):                                   # inf * 0 is there, and gives NaN
            part = spec.view(np.float32).reshape(shape[0], shape[1], -1)
            inf_times_0 = np.isinf(part).any(axis=2) & (masks[0] == 0)
            assert inf_times_0.any() and np.isnan(want[0].view(np.float32).reshape(part.shape)[inf_times_0]).any(axis=1).all()
        run = Launch(par, spec, spec.dtype, shape[1] + 3)
        got = run.run(kind, kernel, power, margin)
        assert same(got[0], want[0]), (cls, kind, power, margin) + where_differs(got[0], want[0])
        if kind == COMPONENTS:
            assert same(got[1], want[1]), (cls, kind, power, margin) + where_differs(got[1], want[1])
        else:
            assert run.untouched(1)                                                         # out_p given, and left alone
            run = Launch(par, spec, spec.dtype)
            alone = run.run(kind, kernel, power, margin, out_p=False)                       # out_p NULL
            assert same(alone[0], want[0]) and run.untouched(1)


# ---------------------------------------------------------------------------------------------------------------- residual
@pytest.mark.parametrize("strides", [(1, 1, 1, 1), (2, 3, 1, 2)], ids=str)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_residual_between_guards(par, n, strides):
    rng = np.random.default_rng(n)
    special = np.float32([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, 3e38, -3e38])
    host = []
    for s in strides[:3]:
        v = rng.standard_normal(n).astype(np.float32)
        at = rng.random(n) < 0.3
        v[at] = rng.choice(special, int(at.sum()))
        flat = np.full((n - 1) * s + 1, SENTINEL, np.float32)
        flat[::s] = v
        host.append((v, flat))
    host[1][0][0], host[2][0][0], host[0][0][0] = np.float32(-0.0), np.float32(0.0), np.float32(-0.0)       # -0 - (-0 + 0) = -0
    for (v, flat), s in zip(host, strides):
        flat[::s] = v
    bufs = [Guarded(par, flat, GUARD, SENTINEL) for _, flat in host]
    rs = strides[3]
    out = Guarded(par, np.full((n - 1) * rs + 1, SENTINEL, np.float32), GUARD, SENTINEL)
    par.check(par.L.par_residual_f32(par.dev, bufs[0].ptr(), strides[0], bufs[1].ptr(), strides[1], bufs[2].ptr(), strides[2], n, out.ptr(), rs,
                                     par.stream()))
    par.torch.cuda.synchronize()
    got = out.read()
    with np.errstate(all="ignore"):
        want = host[0][0] - (host[1][0] + host[2][0])
    assert want.dtype == np.float32 and (n < 20 or (np.isnan(want).any() and np.isinf(want).any()))
    assert same(got[::rs], want), where_differs(got[::rs], want)
    gap = np.ones(len(got), bool)
    gap[::rs] = False
    assert (bits(got)[gap] == SENTINEL_BITS).all() and out.guards_intact() and all(b.unchanged() for b in bufs)
