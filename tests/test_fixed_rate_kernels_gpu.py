"""K_rsfix at the C ABI (par_resample_fixed_f32 of csrc/resample_fixed.hip), kernel form by kernel form, against the float64 statement
of tests/fixed_rate_np.py, where test_fixed_rate_gpu.py (four ratios at num_zeros 8, noise) does not reach: every cell of the
phase-major LDS table of k_rsfix_up<8> and of the natural table of k_rsfix_any, one tap at a time (tests/fixed_rate_inputs.py;
test_fixed_rate_inputs_cpu.py proves the coverage and that a wrong cell is seen); k_rsfix_any<true> at other table sizes and at
ratio < 1, up to the last size that fits LDS (15); k_rsfix_any<false> (16..64); the second trip of both grid-stride loops;
positions past 2^24 on the generic kernel; NaN and inf locality; strides.

Every output is held to fixed_rate_np.tolerance(K, B) = (K + 5) 2^-24 B, derived there and unchanged; where K = 0 or B = 0 that
is an exact 0.  There is no other threshold.  Every call: x lies between guard rows of a NaN with a payload (so does every cell
between strided samples) and must be unchanged afterwards; y is prefilled with that NaN, its guards and the cells between
strided outputs must keep it and every output cell must lose it; every case runs twice and must repeat bit for bit.
pytest -s prints the worst error / bound per case (NOTES.md, Fixed-ratio resampler)."""
import numpy as np
import pytest

import fixed_rate_inputs as I
import fixed_rate_np as F
from test_fixed_rate_gpu import SENTINEL
from test_heal_kernels_gpu import Guarded, bits

pytestmark = pytest.mark.gpu

SENT = np.array([SENTINEL], dtype=np.uint32).view(np.float32)[0]
ANY_CAP = 4 * 256 * 256                  # outputs of one trip of k_rsfix_any's grid: 4 workgroups per CU, 256 CUs, 256 lanes
UP_CAP = 3 * 256 * 512                   # ... of k_rsfix_up's: 3 per CU, 512 lanes


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


def noise(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)


def is_sent(a):
    return bits(a) == SENTINEL


def resample(par, x, a, b, z=8, xs=1, ys=1, xc=0, yc=0, guard=3):
    """par_resample_fixed_f32 on channel xc of xs interleaved ones -> channel yc of ys, from two guarded runs that must agree bit
    for bit.  guard = 3 rows: with an odd stride, or stride 1, x starts at an odd element of its allocation."""
    n = len(x)
    n_out = F.out_len(n, a, b)
    assert par.L.par_resample_fixed_out_len(n, float(a), float(b)) == n_out
    body = np.full((n, xs), SENT, dtype=np.float32)
    body[:, xc] = x
    gx = Guarded(par, body, guard, SENT)
    got = []
    for _ in range(2):
        out = Guarded(par, np.full((n_out, ys), SENT, dtype=np.float32), guard, SENT)
        par.check(par.L.par_resample_fixed_f32(par.dev, gx.ptr(xc), n, xs, float(a), float(b), z, out.ptr(yc), n_out, ys, par.stream()))
        par.torch.cuda.synchronize()
        h = out.read()
        assert out.guards_intact(), "a cell before y[0] or behind y[n_out - 1] was written"
        for c in range(ys):
            if c != yc:
                assert is_sent(h[:, c]).all(), "a cell between strided outputs was written"
        assert not is_sent(h[:, yc]).any(), "an output cell was left unwritten"
        got.append(h[:, yc].copy())
    assert np.array_equal(bits(got[0]), bits(got[1])), "two runs differ"
    assert gx.unchanged(), "the input was written"
    return got[0]


def held(got, y, K, B, label):
    """every output within the derived bound (an exact 0 where the bound is 0) -> worst error / bound"""
    assert got.shape == y.shape and got.dtype == np.float32, label
    tol = F.tolerance(K, B)
    err = np.abs(got.astype(np.float64) - y)
    k = int(np.argmax(err - tol))
    assert np.all(err <= tol), (label, "output", k, "got", float(got[k]), "want", float(y[k]), "error / bound", float(err[k] / tol[k]) if tol[k] else np.inf)
    return float(np.max(err / np.where(tol > 0, tol, 1.0)))


# ------------------------------------------------------------------------------------------------------------------ cell sweep
SWEEP = [(8, I.UP, "k_rsfix_up<8>"), (8, I.DOWN, "k_rsfix_any<true>"), (16, I.UP, "k_rsfix_any<false>"), (16, I.DOWN, "k_rsfix_any<false>"),
         (15, I.DOWN, "k_rsfix_any<true>")]


@pytest.mark.parametrize("z,rates,form", SWEEP, ids=[f"z{z}-{r[0]}-{r[1]}" for z, r, _ in SWEEP])
def test_every_table_cell_one_tap_at_a_time(par, z, rates, form):
    a, b = rates
    pl = I.plan(a, b, z)
    S = I.train_period(z)
    Y, B = I.train_outputs(pl, S)
    worst = 0.0
    for p in range(S):
        got = resample(par, I.train(pl.n, S, p), a, b, z)
        worst = max(worst, held(got, Y[p], pl.K, B[p], (z, a, b, "phase", p)))
        assert np.array_equal(got == 0, Y[p] == 0), (z, a, b, "phase", p, "an output whose taps miss the impulses is an exact 0, and no other")
    print(f"\nK_rsfix cell sweep num_zeros {z}, {a} -> {b} ({form}): {S} trains x {len(pl.K)} outputs, {np.count_nonzero(Y)} single "
          f"weights, worst error / bound {worst:.3f}")


# ----------------------------------------------------------------------------------------------------------- other table sizes
def noise_case(par, a, b, n, z, seed, label, **kw):
    x = noise(n, seed)
    y, K, B = I.plan(a, b, z, n).evaluate(x)
    w = held(resample(par, x, a, b, z, **kw), y, K, B, label)
    print(f"\nK_rsfix {label}: {len(y)} outputs, taps <= {K.max()}, worst error / bound {w:.3f}")
    return K


@pytest.mark.parametrize("z", [1, 7, 9, 15, 16, 64])
@pytest.mark.parametrize("rates", [I.UP, I.DOWN], ids=["up", "down"])
def test_other_table_sizes_near_ratio_one(par, z, rates):
    a, b = rates
    K = noise_case(par, a, b, I.SWEEP_N, z, 200 + z, f"noise num_zeros {z}, {a} -> {b}")
    pl = I.plan(a, b, z)
    x = I.train(pl.n, I.train_period(z), 0)
    y, K, B = pl.evaluate(x)
    got = resample(par, x, a, b, z)
    w = held(got, y, K, B, ("train", z, a, b))
    assert np.array_equal(got == 0, y == 0)
    print(f"K_rsfix phase-0 train num_zeros {z}, {a} -> {b}: {np.count_nonzero(K == 0)} outputs without a tap, worst error / bound {w:.3f}")
    if z == 1 and rates == I.UP:
        assert np.count_nonzero(K == 0) > len(K) // 2           # one tap for off <= 1 only: mostly exact zeros


@pytest.mark.parametrize("z", [15, 16, 64])
def test_a_sixteenth_at_the_lds_limit_and_past_it(par, z):
    """num_zeros 15 is the LDS form at step 32, 16 and 64 the cached form: up to 2047 taps at 64"""
    K = noise_case(par, 16, 1, 3000, z, 300 + z, f"noise num_zeros {z}, 16 -> 1")
    assert K.max() == 32 * z - 1 and K.min() < K.max()


def test_sixteen_up(par):
    noise_case(par, 1, 16, 80, 8, 41, "noise num_zeros 8, 1 -> 16 (k_rsfix_up<8>)")


def test_ratio_one_on_the_generic_kernel(par):
    noise_case(par, 1, 1, 40, 5, 43, "noise num_zeros 5, 1 -> 1 (k_rsfix_any<true>, scale 1)")


def test_just_below_ratio_one(par):
    """rates 1 -> 1 - 2^-52: ratio < 1 by one ulp, so the generic kernel with step 511 and a scale that is not 1"""
    b = 1.0 - 2.0 ** -52
    pl = I.plan(1, b, 8, 40)
    assert pl.scale < 1.0 and pl.step == 511 and len(pl.K) == 39
    noise_case(par, 1, b, 40, 8, 47, "noise num_zeros 8, 1 -> 1 - 2^-52 (k_rsfix_any<true>, step 511)")


# ----------------------------------------------------------------------------------------------------------- second launch trip
TRIPS = [(I.DOWN, 263_000, 8, ANY_CAP, 262_743), (I.DOWN, 263_000, 16, ANY_CAP, 262_743), (I.UP, 394_000, 8, UP_CAP, 394_385)]


@pytest.mark.parametrize("rates,n,z,cap,n_out", TRIPS, ids=["any-lds", "any-cached", "up"])
def test_second_trip_of_the_grid_stride_loop(par, rates, n, z, cap, n_out):
    a, b = rates
    assert F.out_len(n, a, b) == n_out > cap
    x = noise(n, 53 + z)
    got = resample(par, x, a, b, z)                      # asserts: no cell of [0, n_out) keeps the sentinel, the cells behind do
    for t0, t1 in ((cap - 512, n_out), (0, 512)):
        y, K, B = F.Plan(n, a, b, t0, t1, z).evaluate(x)
        w = held(got[t0:t1], y, K, B, (a, b, z, t0, t1))
        print(f"\nK_rsfix second trip num_zeros {z}, {a} -> {b}, n {n}: outputs [{t0}, {t1}) worst error / bound {w:.3f}")


def test_positions_past_2_to_24_on_the_generic_kernel(par):
    n = (1 << 24) + 4099
    a, b = 48000, 44100
    x = noise(n, 7)
    n_out = F.out_len(n, a, b)
    got = resample(par, x, a, b, 8)
    inc = 1.0 / (float(b) / a)
    t_cross = int(np.ceil((1 << 24) / inc))
    while t_cross * inc < (1 << 24):
        t_cross += 1
    assert (t_cross - 1) * inc < (1 << 24) <= t_cross * inc and t_cross + 1024 < n_out - 2048
    for t0, t1 in ((t_cross - 1024, t_cross + 1024), (n_out - 2048, n_out)):
        y, K, B = F.Plan(n, a, b, t0, t1).evaluate(x)
        w = held(got[t0:t1], y, K, B, (t0, t1))
        print(f"\nK_rsfix positions past 2^24, 48000 -> 44100: outputs [{t0}, {t1}) worst error / bound {w:.3f}")


# -------------------------------------------------------------------------------------------------------------------- locality
FORMS = [(8, I.UP, "k_rsfix_up<8>"), (8, I.DOWN, "k_rsfix_any<true>"), (16, I.UP, "k_rsfix_any<false>")]


@pytest.mark.parametrize("z,rates,form", FORMS, ids=["up", "any-lds", "any-cached"])
def test_a_nan_or_an_inf_stays_in_the_outputs_whose_taps_hold_it(par, z, rates, form):
    """x's guard cells x[-1] and x[n] hold NaN in every run here (the sentinel is one): the clean run must be finite."""
    a, b = rates
    pl = I.plan(a, b, z)
    q = I.NAN_Q
    hit, left, right = I.nan_map(pl, q)
    x = noise(pl.n, 61 + z)
    x[q] = 0.0
    clean = resample(par, x, a, b, z)
    assert np.all(np.isfinite(clean))
    y, K, B = pl.evaluate(x)
    held(clean, y, K, B, (form, "clean"))
    for poison in (np.float32(np.nan), np.float32(np.inf)):
        x[q] = poison
        got = resample(par, x, a, b, z)
        assert np.array_equal(~np.isfinite(got), hit), (form, float(poison), np.nonzero(~np.isfinite(got))[0], np.nonzero(hit)[0])
        assert np.array_equal(bits(got[~hit]), bits(clean[~hit])), (form, float(poison), "an output whose taps miss x[q] changed")
        if np.isinf(poison):                             # one inf times one non-zero weight: an inf, not a NaN
            assert np.all(np.isinf(got[hit]))
    print(f"\nK_rsfix locality {form}: x[{q}] reaches outputs {np.nonzero(left)[0].tolist()} (left wing) and {np.nonzero(right)[0].tolist()} (right)")


# --------------------------------------------------------------------------------------------------------------------- strides
@pytest.mark.parametrize("xs,ys,xc,yc", [(3, 5, 2, 3), (1, 2, 0, 1)], ids=["3-5", "1-2"])   # x starts at element 11 and 3
@pytest.mark.parametrize("z,rates,form", FORMS, ids=["up", "any-lds", "any-cached"])
def test_strides_and_an_odd_start(par, z, rates, form, xs, ys, xc, yc):
    a, b = rates
    noise_case(par, a, b, I.SWEEP_N, z, 71 + z, f"noise {form} x_stride {xs} y_stride {ys}", xs=xs, ys=ys, xc=xc, yc=yc)
