"""par_crossing_smooth_f64 and par_interp_f64 at the C ABI, on the GPU.

The yardsticks are tests/zerocross_np.py: the exact sum (integers times float64 weights, summed without rounding, rounded once)
for `smooth` and `freq`, numpy itself for `xp`, `raw` and the interpolation.  Bounds (derived in zerocross_np's docstring, none
measured): |smooth - exact| <= (span + 2) 2^-53 exact for any summation order, since every term is non-negative; freq the same
with span + 4 (one more division, and smooth's error through 1 / x); xp, raw and par_interp_f64 bit for bit.  Every output lies
between sentinel cells and is NaN-filled first, every call is made twice and must give identical bits."""
import ctypes
import math

import numpy as np
import pytest

import zerocross_np as Z

pytestmark = pytest.mark.gpu
T = 256                      # outputs per K_zcsmooth workgroup (csrc/crossings.hip kZcsTile)
BLOCK = 256                  # threads per K_interp workgroup
MAX_SPAN = 4096              # PAR_CROSSING_SMOOTH_MAX_SPAN
GUARD = 8
SENTINEL = -777.25
SR, T0 = 192000.0, 1.7


@pytest.fixture(scope="module")
def par():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    from pyaudiorestoration_amd import _dev, _lib

    class P:
        pass
    p = P()
    p.torch, p.dev, p.L, p.lib, p.stream, p.ptr = torch, 0, _lib.lib(), _lib, lambda: _dev.stream_ptr(0), _dev.ptr
    assert _lib.CROSSING_SMOOTH_MAX_SPAN == MAX_SPAN
    return p


class Guarded:
    """a device array of n cells, NaN-filled, between GUARD sentinel cells on each side"""
    def __init__(self, par, n, dtype):
        self.full = par.torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda:0")
        self.view = self.full[GUARD:GUARD + n]
        self.view.fill_(float("nan"))
        self.n = n

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def read(self):
        h = self.full.cpu().numpy()
        assert np.all(h[:GUARD] == SENTINEL) and np.all(h[GUARD + self.n:] == SENTINEL), "a sentinel cell was written"
        return h[GUARD:GUARD + self.n].copy()


def bits(a):
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def smooth_call(par, crossings, span, sr=SR, t0=T0, kernel=None):
    """-> (smooth, freq, xp, raw) of one call, after checking that a second call gives the same bits"""
    torch = par.torch
    c = len(crossings)
    n = c - 1
    c_t = torch.from_numpy(np.ascontiguousarray(crossings, dtype=np.int64)).to("cuda:0")
    k_t = torch.from_numpy(Z.hann_kernel(span) if kernel is None else kernel).to("cuda:0")
    got = []
    for _ in range(2):
        outs = [Guarded(par, n, torch.float64) for _ in range(3)] + [Guarded(par, n, torch.float32)]
        rc = par.L.par_crossing_smooth_f64(0, par.ptr(c_t), c, par.ptr(k_t), span, sr, t0, outs[0].ptr(), outs[1].ptr(), outs[2].ptr(),
                                           outs[3].ptr(), par.stream())
        assert rc == 0, par.lib.last_error()
        torch.cuda.synchronize()
        got.append([o.read() for o in outs])
    for a, b in zip(*got):
        assert np.array_equal(bits(a), bits(b)), "two runs differ"
    return got[0]


def make_periods(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "constant":
        return np.full(n, 24, dtype=np.int64)
    if kind == "long":                                    # a single long period among ones
        d = np.ones(n, dtype=np.int64)
        d[n // 2] = 1000
        return d
    d = rng.integers(1, 41, n).astype(np.int64)
    if kind == "gap":                                     # one gap above 2^24 samples: its float32 rounds (2^24 + 3 -> 2^24 + 4)
        d[n // 3] = (1 << 24) + 3
    return d


def crossings_of(d, first=5):
    return np.concatenate(([first], first + np.cumsum(d))).astype(np.int64)


def spans_for(n):
    """1, 2, 3: both parities of the centring; n - 1, n, n + 1, 2 (n - 1) + 1: single, exact and repeated reflection"""
    return sorted({s for s in (1, 2, 3, n - 1, n, n + 1, 2 * (n - 1) + 1) if 1 <= s <= MAX_SPAN})


NS = (2, 3, T - 1, T, T + 1, 2 * T + 1)
KINDS = ("constant", "long", "random", "gap")
CASES = [(n, span, kind) for n in NS for span in spans_for(n) for kind in KINDS]
CASES += [(n, MAX_SPAN, kind) for n in (3, T + 1) for kind in KINDS]


def check_against_the_yardsticks(got, crossings, span, sr, t0):
    smooth, freq, xp, raw = got
    d = Z.periods(crossings)
    n = len(d)
    kernel = Z.hann_kernel(span)
    exact = Z.exact_smooth(d, kernel)
    assert smooth.shape == (n,) and np.all(np.isfinite(smooth))
    err = np.abs(smooth - exact)
    print(f"n {n} span {span}: smooth worst {np.max(err / exact) / Z.U:.3f} u of {span + 2}")
    assert np.all(err <= Z.bound_smooth(span) * exact)
    exact_f = (sr / 2) / exact
    errf = np.abs(freq - exact_f)
    print(f"n {n} span {span}: freq worst {np.max(errf / exact_f) / Z.U:.3f} u of {span + 4}")
    assert np.all(errf <= Z.bound_freq(span) * exact_f)
    assert np.array_equal(bits(freq), bits((sr / 2) / smooth))                       # one division of the kernel's own sum
    assert np.array_equal(bits(xp), bits(crossings[:n] / sr + t0))                   # numpy's two roundings
    want_raw = np.float32(sr / 2) / d
    assert want_raw.dtype == np.float32 and np.array_equal(bits(raw), bits(want_raw))
    ref = Z.numpy_chain(crossings, sr, span, t0)                                     # the reference's statement, numpy's order
    assert np.all(np.abs(freq - ref["freq"]) <= Z.bound_vs_numpy(span) * ref["freq"])
    return d, kernel, exact


@pytest.mark.parametrize("n,span,kind", CASES, ids=[f"n{n}_span{s}_{k}" for n, s, k in CASES])
def test_crossing_smooth_holds_the_derived_bounds(par, n, span, kind):
    """n around the tile (one workgroup, a partial one, more than one), spans from no smoothing to the largest supported, with
    pads narrower than, equal to and wider than the array.  Bounds: module docstring."""
    d_int = make_periods(kind, n, seed=n * 7 + span)
    crossings = crossings_of(d_int)
    got = smooth_call(par, crossings, span)
    d, kernel, exact = check_against_the_yardsticks(got, crossings, span, SR, T0)
    smooth = got[0]
    if kind == "constant":                                # the constant times the sum of the weights, within the same bound
        want = 24.0 * math.fsum(kernel)
        assert np.all(np.abs(smooth - want) <= Z.bound_smooth(span) * want)
    if span == 1:                                         # the reference's quirk, kept: the single Hann weight is 2
        assert np.array_equal(smooth, 2.0 * d.astype(np.float64))
    if kind == "gap":
        assert d[n // 3] == np.float32((1 << 24) + 4)


@pytest.mark.parametrize("n,span", [(3, 2), (T + 1, 3), (T + 1, T + 2), (2 * T + 1, 81)])
def test_crossing_indices_above_2_to_the_32(par, n, span):
    """64-bit crossing indices: the periods are differences in int64, xp is still numpy's bits"""
    d_int = make_periods("random", n, seed=n + span)
    crossings = crossings_of(d_int, first=(1 << 32) + 12345)
    assert crossings[0] > 1 << 32
    check_against_the_yardsticks(smooth_call(par, crossings, span), crossings, span, SR, T0)
    crossings = crossings_of(d_int, first=(1 << 40) + 1)              # and a sample rate / offset of another scale
    check_against_the_yardsticks(smooth_call(par, crossings, span, 44100.0, 0.0), crossings, span, 44100.0, 0.0)


def test_crossing_smooth_optional_outputs(par):
    """smooth and raw may be null; freq and xp are the same bits either way"""
    torch = par.torch
    crossings = crossings_of(make_periods("random", T + 1, seed=1))
    full = smooth_call(par, crossings, 5)
    c_t = torch.from_numpy(crossings).to("cuda:0")
    k_t = torch.from_numpy(Z.hann_kernel(5)).to("cuda:0")
    freq, xp = Guarded(par, T + 1, torch.float64), Guarded(par, T + 1, torch.float64)
    assert par.L.par_crossing_smooth_f64(0, par.ptr(c_t), len(crossings), par.ptr(k_t), 5, SR, T0, None, freq.ptr(), xp.ptr(), None,
                                         par.stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(freq.read()), bits(full[1])) and np.array_equal(bits(xp.read()), bits(full[2]))


def test_crossing_smooth_argument_errors_leave_the_outputs_alone(par):
    torch = par.torch
    crossings = crossings_of(make_periods("random", 10, seed=2))
    c_t = torch.from_numpy(crossings).to("cuda:0")
    k_t = torch.from_numpy(Z.hann_kernel(3)).to("cuda:0")
    outs = [Guarded(par, 10, torch.float64) for _ in range(3)] + [Guarded(par, 10, torch.float32)]
    good = dict(crossings=par.ptr(c_t), c=11, kernel=par.ptr(k_t), span=3, sr=SR)
    bad = [dict(crossings=None), dict(kernel=None), dict(c=2), dict(c=0), dict(span=0), dict(span=-1), dict(span=MAX_SPAN + 1),
           dict(sr=0.0), dict(sr=-48000.0), dict(sr=float("nan")), dict(sr=float("inf"))]
    for change in bad:
        a = dict(good, **change)
        rc = par.L.par_crossing_smooth_f64(0, a["crossings"], a["c"], a["kernel"], a["span"], a["sr"], T0, outs[0].ptr(), outs[1].ptr(),
                                           outs[2].ptr(), outs[3].ptr(), par.stream())
        assert rc == 1, change
    for null in (1, 2):                                   # freq and xp are required
        ptrs = [o.ptr() for o in outs]
        ptrs[null] = None
        assert par.L.par_crossing_smooth_f64(0, good["crossings"], 11, good["kernel"], 3, SR, T0, *ptrs, par.stream()) == 1
    torch.cuda.synchronize()
    for o in outs:
        assert np.all(np.isnan(o.read()))


# ------------------------------------------------------------------------------------------------------------- par_interp_f64
def interp_call(par, x, xp, fp):
    torch = par.torch
    x, xp, fp = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, xp, fp))
    xp_t, fp_t = torch.from_numpy(xp).to("cuda:0"), torch.from_numpy(fp).to("cuda:0")
    x_t = torch.from_numpy(x).to("cuda:0") if len(x) else torch.empty(1, dtype=torch.float64, device="cuda:0")
    got = []
    for _ in range(2):
        out = Guarded(par, len(x), torch.float64)
        rc = par.L.par_interp_f64(0, par.ptr(x_t), len(x), par.ptr(xp_t), par.ptr(fp_t), len(xp), out.ptr(), par.stream())
        assert rc == 0, par.lib.last_error()
        torch.cuda.synchronize()
        got.append(out.read())
    assert np.array_equal(bits(got[0]), bits(got[1]))
    return got[0]


def assert_numpys_bits(got, x, xp, fp):
    want = np.interp(x, xp, fp)
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert got.shape == want.shape and np.all(same), (np.asarray(x)[~same], got[~same], want[~same])


def around(xp):
    """below, on and above every knot"""
    xp = np.asarray(xp, dtype=np.float64)
    return np.concatenate([np.nextafter(xp, -np.inf), xp, np.nextafter(xp, np.inf), xp - 0.37, xp + 0.41, [xp[0] - 1e9, xp[-1] + 1e9]])


@pytest.mark.parametrize("m", [1, 2, 7, BLOCK - 1, BLOCK + 1])
def test_interp_around_every_knot(par, m):
    rng = np.random.default_rng(m)
    xp = np.cumsum(rng.uniform(0.1, 2.0, m)) - 3.0
    fp = rng.standard_normal(m) * 1000.0
    x = around(xp)
    rng.shuffle(x)                                        # x in no order
    assert_numpys_bits(interp_call(par, x, xp, fp), x, xp, fp)
    x = np.concatenate([x, [np.nan, np.inf, -np.inf]])    # a NaN abscissa is NaN (one knot: fp[0]), as numpy's
    assert_numpys_bits(interp_call(par, x, xp, fp), x, xp, fp)


def test_interp_equal_knots_take_the_last(par):
    xp = np.array([0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 3.0])
    fp = np.array([10.0, 11.0, 12.0, 13.0, 14.0, 15.0, 16.0])
    x = around(xp)
    got = interp_call(par, x, xp, fp)
    assert_numpys_bits(got, x, xp, fp)
    assert interp_call(par, [1.0], xp, fp)[0] == 13.0 and interp_call(par, [2.0], xp, fp)[0] == 15.0
    xp = np.array([1.0, 1.0, 1.0])                       # nothing but one abscissa
    assert_numpys_bits(interp_call(par, around(xp), xp, fp[:3]), around(xp), xp, fp[:3])


@pytest.mark.parametrize("fp", [[1.0, np.nan, 3.0, 4.0, 5.0], [np.inf, np.inf, 1.0, -np.inf, 2.0], [np.nan, 1.0, 2.0, 3.0, np.nan],
                                [1.0, np.inf, -np.inf, np.inf, 0.0], [-np.inf, -np.inf, -np.inf, 0.0, np.inf]],
                         ids=["nan_inside", "inf_pair", "nan_ends", "inf_alternating", "inf_run"])
def test_interp_nan_and_inf_in_fp_propagate_as_numpys(par, fp):
    xp = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    x = np.concatenate([around(xp), np.linspace(-0.5, 4.5, 41)])
    with np.errstate(all="ignore"):
        assert_numpys_bits(interp_call(par, x, xp, fp), x, xp, fp)


@pytest.mark.parametrize("nx", [0, 1, BLOCK - 1, BLOCK + 1, 3 * BLOCK + 5])
def test_interp_lengths_around_the_block(par, nx):
    rng = np.random.default_rng(nx)
    xp = np.sort(rng.uniform(0.0, 10.0, 50))
    fp = rng.standard_normal(50)
    x = rng.uniform(-1.0, 11.0, nx)
    got = interp_call(par, x, xp, fp)
    assert got.shape == (nx,)
    assert_numpys_bits(got, x, xp, fp)


def test_interp_argument_errors(par):
    torch = par.torch
    t = torch.zeros(4, dtype=torch.float64, device="cuda:0")
    out = Guarded(par, 4, torch.float64)
    p = par.ptr(t)
    assert par.L.par_interp_f64(0, p, 4, p, p, 0, out.ptr(), par.stream()) == 1           # m < 1
    assert par.L.par_interp_f64(0, p, -1, p, p, 4, out.ptr(), par.stream()) == 1          # nx < 0
    for args in ((None, 4, p, p, 4, out.ptr()), (p, 4, None, p, 4, out.ptr()), (p, 4, p, None, 4, out.ptr()), (p, 4, p, p, 4, None)):
        assert par.L.par_interp_f64(0, *args, par.stream()) == 1
    assert par.L.par_interp_f64(0, p, 0, p, p, 4, out.ptr(), par.stream()) == 0           # nx == 0: nothing done
    torch.cuda.synchronize()
    assert np.all(np.isnan(out.read()))
