"""K_lerp and K_lag at the C ABI (par_linear_resample_f32, par_lag_to_pos_f64 of csrc/lag.hip), bit for bit against np.interp,
where the wrapper-level tests (one golden at 1e-6, three random curves) do not reach: positions on samples, on the last sample
and one ulp beside both ends, outside the signal, infinite and NaN; samples that are infinite, NaN, denormal or signed zeros,
met on the knot and between knots; a one-sample signal; strides; K_lag's cutoff on a block's first lane, a wave's last lane, in
a partial last block and absent; held ends, equal knots, values below 0 and a curve that crosses the signal's length twice.

Every buffer lies between guard rows of a sentinel, outputs are prefilled with it, inputs must be unchanged, and every case runs
twice and must repeat bit for bit.  There is no tolerance in this file."""
import ctypes

import numpy as np
import pytest

from test_fixed_rate_gpu import SENTINEL
from test_heal_kernels_gpu import Guarded, bits

pytestmark = pytest.mark.gpu

SENT32 = np.array([SENTINEL], dtype=np.uint32).view(np.float32)[0]
SENT64 = np.array([0x7FF8000012345678], dtype=np.uint64).view(np.float64)[0]


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


def same(got, want):
    """bit for bit, except that a NaN equals any NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


# ------------------------------------------------------------------------------------------------------------------- K_lerp
def lerp(par, pos, sig, ss=1, os_=1):
    len_out, len_in = len(pos), len(sig)
    body = np.full((len_in, ss), SENT32, dtype=np.float32)
    body[:, ss - 1] = sig
    gs = Guarded(par, body, 3, SENT32)
    gp = Guarded(par, np.asarray(pos, dtype=np.float64), 3, SENT64)
    got = []
    for _ in range(2):
        out = Guarded(par, np.full((len_out, os_), SENT32, dtype=np.float32), 3, SENT32)
        par.check(par.L.par_linear_resample_f32(par.dev, gp.ptr(), len_out, gs.ptr(ss - 1), ss, len_in, out.ptr(os_ - 1), os_, par.stream()))
        par.torch.cuda.synchronize()
        h = out.read()
        assert out.guards_intact()
        for c in range(os_ - 1):
            assert np.all(bits(h[:, c]) == SENTINEL), "a cell between strided outputs was written"
        assert not np.any(bits(h[:, os_ - 1]) == SENTINEL), "an output cell was left unwritten"
        got.append(h[:, os_ - 1].copy())
    assert np.array_equal(bits(got[0]), bits(got[1])), "two runs differ"
    assert gs.unchanged() and gp.unchanged()
    return got[0]


def lerp_ref(pos, sig):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.interp(pos, np.arange(len(sig), dtype=np.float64), sig.astype(np.float64), left=0, right=0).astype(np.float32)


PAIRS = [(np.inf, np.inf), (np.inf, -np.inf), (np.nan, 1.0), (1.0, np.nan)]
PAIR_AT = (10, 20, 30, 40)               # where a long signal holds the pairs; 50.. hold denormals, signed zeros and a lone -inf


def lerp_signal(len_in, variant=0):
    sig = np.random.default_rng(500 + len_in).uniform(-1, 1, len_in).astype(np.float32)
    if len_in == 1:
        sig[0] = (0.7, np.inf, np.nan)[variant]
    elif len_in == 2:
        sig[:] = PAIRS[variant]
    else:
        for at, pair in zip(PAIR_AT, PAIRS):
            sig[at:at + 2] = pair
        sig[50:52] = (1e-40, -3e-42)                              # float32 denormals, and between them
        sig[60:62] = (0.0, -0.0)
        sig[70] = -np.inf
        sig[len_in - 1] = 0.375                                   # the end itself stays a plain value ...
        sig[0] = -0.625
    return sig


def lerp_positions(len_in):
    """The table: specials first (so a short call still meets them), then every sample, then fractions."""
    last = float(len_in - 1)
    head = [0.0, -0.0, last, np.nextafter(0.0, -1.0), np.nextafter(0.0, 1.0), np.nextafter(last, -np.inf), np.nextafter(last, np.inf),
            np.nan, np.inf, -np.inf, -1.0, -0.5, -1e300, last + 0.5, last + 1.0, 1e300, float(len_in)]
    if len_in > 2:
        for at in PAIR_AT + (50, 60, 69, 70):                     # each pair on its knots and between them
            head += [float(at), at + 1.0, at + 0.5, at + 0.25, np.nextafter(at + 1.0, 0.0), np.nextafter(float(at), np.inf)]
    rng = np.random.default_rng(600 + len_in)
    frac = rng.uniform(0, max(last, 1.0), 300)
    body = np.concatenate([np.arange(len_in, dtype=np.float64), frac, np.sort(frac)[::-1], np.repeat(frac[:20], 3),
                           rng.uniform(-2, last + 2, 100)])
    return np.concatenate([np.array(head, dtype=np.float64), body])


LERP_IN = [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (2, 3), (257, 0), (5000, 0)]


@pytest.mark.parametrize("len_in,variant", LERP_IN, ids=[f"in{n}-v{v}" for n, v in LERP_IN])
@pytest.mark.parametrize("ss,os_", [(1, 1), (2, 2), (3, 1)], ids=["1-1", "2-2", "3-1"])
def test_lerp_is_np_interp_bit_for_bit(par, len_in, variant, ss, os_):
    sig = lerp_signal(len_in, variant)
    table = lerp_positions(len_in)
    for len_out in (1, 255, 256, 257, 4099, len(table)):          # the whole table too: every sample of the longest signal
        pos = np.resize(table, len_out)
        want = lerp_ref(pos, sig)
        got = lerp(par, pos, sig, ss, os_)
        bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))[0]
        assert same(got, want), (len_in, variant, len_out, "first at", int(bad[0]), "pos", float(pos[bad[0]]), "got", float(got[bad[0]]),
                                 "want", float(want[bad[0]]))
    if len_in > 2:                                                # the table did meet what it is for
        want = lerp_ref(table, sig)
        assert np.isnan(want).sum() > 10 and np.isinf(want).sum() > 10 and np.any((want != 0) & (np.abs(want) < 1e-38))
        assert np.any(bits(want) == 0x80000000)                   # the -0 sample, on its knot


# -------------------------------------------------------------------------------------------------------------------- K_lag
def lag(par, xp, fp, num_out, len_signal):
    """-> (pos[:len_out], len_out, trimmed) from two guarded runs"""
    gx = Guarded(par, np.asarray(xp, dtype=np.float64), 3, SENT64)
    gf = Guarded(par, np.asarray(fp, dtype=np.float64), 3, SENT64)
    got = []
    for _ in range(2):
        out = Guarded(par, np.full(num_out, SENT64), 3, SENT64)
        work = Guarded(par, np.full(1, -1, dtype=np.int64), 3, np.int64(-1))
        len_out, trimmed = ctypes.c_int64(-5), ctypes.c_int(-5)
        par.check(par.L.par_lag_to_pos_f64(par.dev, gx.ptr(), gf.ptr(), len(xp), num_out, int(len_signal), out.ptr(), work.ptr(),
                                           ctypes.byref(len_out), ctypes.byref(trimmed), par.stream()))
        par.torch.cuda.synchronize()
        h = out.read()
        assert out.guards_intact() and work.guards_intact()
        assert 0 <= len_out.value <= num_out
        got.append((h[:len_out.value].copy(), len_out.value, trimmed.value))
    assert np.array_equal(bits(got[0][0]), bits(got[1][0])) and got[0][1:] == got[1][1:], "two runs differ"
    assert gx.unchanged() and gf.unchanged()
    return got[0]


def lag_ref(xp, fp, num_out, len_signal):
    full = np.interp(np.arange(num_out), xp, fp)
    over = np.nonzero(full >= len_signal)[0]
    len_out = int(over[0]) if len(over) else num_out
    return np.clip(full[:len_out], 0, None), len_out, int(len(over) > 0), full


def check_lag(par, xp, fp, num_out, len_signal, label):
    want, len_out, trimmed, full = lag_ref(xp, fp, num_out, len_signal)
    assert not np.any(np.isnan(full)) and not np.any(full == 0), "the reference is pinned on curves without NaN and without an exact 0"
    got, got_len, got_trimmed = lag(par, xp, fp, num_out, len_signal)
    assert (got_len, got_trimmed) == (len_out, trimmed), (label, "len_out, trimmed", got_len, got_trimmed, "want", len_out, trimmed)
    assert np.array_equal(bits(got), bits(want)), (label, "first at", int(np.nonzero(bits(got) != bits(want))[0][0]))
    return len_out, full


def rising_curve(m, num_out, seed):
    """m knots over the whole of [0, num_out - 1], every slope in [1.2, 3]: the values rise by more than 1 per output, so any
    output can be made the first one at or above an integer len_signal"""
    top = float(max(num_out - 1, 1))
    rng = np.random.default_rng(seed)
    if m == 2:
        xp = np.array([0.0, top])
    else:
        xp = np.concatenate([[0.0], np.sort(rng.uniform(0, top, m - 2)), [top]])
    slope = rng.uniform(1.2, 3.0, m - 1)
    fp = 0.25 + np.concatenate([[0.0], np.cumsum(slope * np.diff(xp))])
    return xp, fp


@pytest.mark.parametrize("num_out", [1, 255, 256, 257, 100_003])
def test_lag_cutoff_at_every_seam(par, num_out):
    """the cutoff (atomicMin over the waves' minima) on a block's first lane, a wave's last and first lane, a block's last lane, the
    next block's first, the last output (a partial last block), and absent"""
    for m in (2, 500):
        xp, fp = rising_curve(m, num_out, 700 + m + num_out)
        full = np.interp(np.arange(num_out), xp, fp)
        assert np.all(np.diff(full) > 1.0)
        for cut in sorted({c for c in (0, 63, 64, 255, 256, num_out - 1) if c < num_out}) + [None]:
            len_signal = int(np.floor(full[cut])) if cut is not None else int(full[-1]) + 2
            len_out, _ = check_lag(par, xp, fp, num_out, len_signal, (m, num_out, cut))
            assert len_out == (num_out if cut is None else cut)


@pytest.mark.parametrize("num_out", [1, 255, 257, 100_003])
def test_lag_held_ends_equal_knots_and_negative_values(par, num_out):
    top = float(max(num_out - 1, 1))
    rng = np.random.default_rng(800 + num_out)
    for m in (2, 500):
        # held ends: xp[0] > 0 and xp[m - 1] < num_out - 1; the curve starts below 0 (strictly: no exact 0) and rises
        xp = np.sort(rng.uniform(0.1 * top, 0.9 * top, m)) if num_out > 1 else np.linspace(0.25, 0.75, m)
        fp = -7.3 + np.concatenate([[0.0], np.cumsum(rng.uniform(0.0, 2.0 * top / m + 1.0, m - 1))])
        for len_signal in (max(int(fp[-1]) + 2, 1), max(int(fp[m // 2]) + 1, 0)):   # absent, and somewhere inside
            len_out, full = check_lag(par, xp, fp, num_out, len_signal, ("held", m, num_out, len_signal))
        assert xp[0] > 0 and xp[-1] < top and np.any(full < 0)
    if num_out > 100:
        # two and three equal knots, on integers (an output falls on them) and off them; fp jumps there
        xp = np.array([0.0, 10.0, 10.0, 20.5, 20.5, 30.0, 30.0, 30.0, 41.25, 41.25, 41.25, top])
        fp = np.array([0.5, 12.0, 14.0, 25.0, 21.0, 33.0, 35.5, 38.0, 50.0, 47.0, 55.0, 3.0 * top])
        for len_signal in (10 ** 9, 36, 38):
            check_lag(par, xp, fp, num_out, len_signal, ("equal knots", num_out, len_signal))


def test_lag_first_of_two_crossings_wins(par):
    num_out = 1000
    xp = np.array([0.0, 300.0, 600.0, 999.0])
    fp = np.array([10.5, 700.5, 100.5, 900.5])
    for len_signal, first in ((500, None), (650, None), (10 ** 6, 1000)):
        len_out, full = check_lag(par, xp, fp, num_out, len_signal, ("twice", len_signal))
        over = full >= len_signal
        if first is None:
            runs = np.count_nonzero(np.diff(over.astype(int)) == 1) + int(over[0])
            assert runs == 2 and len_out == int(np.argmax(over)) < 300             # two separate stretches above; the first one cuts
            assert np.nonzero(over)[0][-1] > 600
        else:
            assert len_out == first
