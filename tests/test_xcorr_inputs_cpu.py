"""Preconditions of tests/test_xcorr_gpu.py, on the CPU: the float64 oracles of tests/xcorr_inputs.py alone.  Every builder has its
peak on the lag it names, every repeated-template case lists exactly the rivals it is built for with a margin the oracle resolves,
the size-class shapes land in the transform size they name, and the two oracles agree with each other.  pytest -s prints the measured
figures (NOTES.md, Correlation)."""
import time

import numpy as np
import pytest

import xcorr_inputs as X

T0 = time.perf_counter()


def test_exact_at_equals_same_direct():
    """fsum at single lags == scipy's direct summation within delta_f, in 'same' and 'full' indexing, on every small shape family
    the GPU tests use (nb > na and nb << na included)"""
    import scipy.signal
    worst = 0.0
    for na, nb in X.EDGE_SHAPES + ((7, 7), (64, 9), (333, 1)):
        a, b = X.signal_pair("white", na, nb)
        same = X.same_direct(a, b)
        assert same.shape == (na,)
        err = float(np.max(np.abs(X.exact_at(a, b, range(na)) - same)))
        full = scipy.signal.correlate(X.normalised(a), X.normalised(b), mode="full", method="direct")
        errf = float(np.max(np.abs(X.exact_at(a, b, range(na + nb - 1), full=True) - full)))
        assert np.max(np.abs(full[(nb - 1) // 2:(nb - 1) // 2 + na] - same)) <= X.delta_f(nb)     # 'same' is 'full' from (nb-1)//2
        worst = max(worst, err / X.delta_f(nb), errf / X.delta_f(nb))
        assert err <= X.delta_f(nb) and errf <= X.delta_f(nb), (na, nb, err, errf)
    print(f"\nexact_at against same_direct: worst {worst:.3f} of delta_f")


@pytest.mark.parametrize("na,nb", X.EDGE_SHAPES)
def test_edge_lag_builders_peak_where_they_say(na, nb):
    for want in X.edge_peaks(na) + (na - 1,):
        a, b = X.edge_case(na, nb, want)
        same = X.same_direct(a, b)
        for v in (same, np.abs(same)):
            assert int(np.argmax(v)) == want, (na, nb, want)
            top, rivals = X.rivals_of(v)
            assert top == want and len(rivals) == 0          # no rival peak: these cases exercise the refinement alone
            assert v[want] - np.max(np.delete(v, want)) > 0.9
        if want == na - 1:
            with pytest.raises(IndexError):
                X.oracle_delay(a, b)
        else:
            o = X.oracle_delay(a, b)
            assert o.peak == want and abs(o.f0 - same[want]) <= X.delta_f(nb)
            assert abs(o.fm - same[want - 1]) <= X.delta_f(nb)            # want == 0: same[-1], the wrapped read


def test_sectioned_edge_lag_builders_peak_where_they_say():
    """the same in the sectioned regime (2 x 2 section pairs, the float64 'full' array under the peak stage): lag 0 and lag na-2 under
    both ignore_phase settings, no rival, and the 4 x bounds the GPU test holds; a peak on na-1 is the IndexError"""
    na, nb = X.SECTIONED_SHAPES[0]
    assert X.section_counts(na, nb) == (2, 2) and X.sectioned_edge_peaks() == (0, na - 2)
    for want in X.sectioned_edge_peaks():
        a, b = X.edge_case(na, nb, want)
        same = X.same_fft(a, b)
        for ign, v in ((False, same), (True, np.abs(same))):
            top, rivals = X.rivals_of(v)
            assert top == want and len(rivals) == 0
            o = X.oracle_delay(a, b, ign)
            bd, bc = X.delay_bounds(o.fm, o.f0, o.fp, nb)
            print(f"\nsectioned edge lag {want} ign {ign}: 4 x bounds {4 * bd:.3e} samples, {4 * bc:.3e} corr", end="")
            assert o.peak == want and 4 * bd < 2e-9 and 4 * bc < 1e-9
    a, b = X.edge_case(na, nb, na - 1)
    assert int(np.argmax(X.same_fft(a, b))) == na - 1
    with pytest.raises(IndexError):
        X.oracle_delay(a, b)


def test_scratch_shapes_cover_the_layouts():
    """the smallest transform, the smallest member of the next size (the most spare room in the transform arrays), the sectioned form"""
    assert [X.xc_fft_len(na, nb) for na, nb in X.SCRATCH_SHAPES] == [1 << 13, 1 << 14, 1 << 20]
    assert [X.section_counts(na, nb) for na, nb in X.SCRATCH_SHAPES] == [(1, 1), (1, 1), (2, 2)]
    na, nb = X.SCRATCH_SHAPES[1]
    assert na + nb - 1 == (1 << 13) + 1


def _rival_checks(a, b, lags, loud, K, ignore_phase=False):
    same = X.same_fft(a, b)
    v = np.abs(same) if ignore_phase else same
    top, rivals = X.rivals_of(v)
    assert top == lags[loud] == int(np.argmax(v)), (K, loud, top)
    assert sorted(rivals) == sorted(np.delete(lags, loud)), (K, loud)                 # exactly K - 1, each ON a copy
    assert np.all(v[top] - v[rivals] < X.RIVAL_TOL) and np.all(np.abs(rivals - top) > 2)
    ex = np.abs(X.exact_at(a, b, lags))
    margin = float(ex[loud] - np.max(np.delete(ex, loud)))
    assert margin >= 100.0 * X.delta_f(len(b)), (K, loud, margin)
    assert X.oracle_delay(a, b, ignore_phase).peak == lags[loud]
    return margin


@pytest.mark.parametrize("K", X.RIVAL_KS)
def test_rival_builders(K):
    for loud in X.rival_positions(K):
        a, b, lags = X.rival_case(K, loud)
        assert len(a) == len(b) == 8000 + 450 * K and len(lags) == K
        margin = _rival_checks(a, b, lags, loud, K)
        print(f"\nK = {K:2d}, louder copy {loud:2d}: margin {margin:.3e} = {margin / X.delta_f(len(b)):.0f} delta_f", end="")


def test_rival_builder_variants():
    """the plateau case lists 64 rivals; the inverted louder copy wins only under ignore_phase; the equal pair ties exactly and the
    oracle gives it to the lower lag; the sectioned pair needs section pairs and sits 400 000 lags apart"""
    a, b, lags = X.rival_case(65, 40)
    top, rivals = X.rivals_of(X.same_fft(a, b))
    assert top == lags[40] and len(rivals) == 64
    a, b, lags = X.rival_case(2, 1, scale=-(1.0 + X.LOUDER))
    _rival_checks(a, b, lags, 1, 2, ignore_phase=True)
    assert X.oracle_delay(a, b, False).peak == lags[0]
    a, b, lags = X.rival_case(2, 1, scale=1.0)
    ex = X.exact_at(a, b, lags)
    assert ex[0] == ex[1] and X.oracle_delay(a, b).peak == lags[0]
    a, b, lags = X.sectioned_rival_case()
    assert X.section_counts(len(a), len(b)) == (2, 2) and lags[1] - lags[0] == 400_000
    margin = _rival_checks(a, b, lags, 1, 2)
    print(f"\nsectioned pair: margin {margin:.3e} = {margin / X.delta_f(len(b)):.0f} delta_f")


def test_size_classes_land_where_they_say():
    def fft_len(na, nb):                                 # the rule of xc_fft_len, restated
        N = 8192
        while N < na + nb - 1 and N < 2 ** 20:
            N <<= 1
        return N
    cases = X.size_classes()
    assert len(cases) == 16 and sorted({c[0] for c in cases}) == [1 << k for k in range(13, 21)]
    for N, kind, na, nb in cases:
        assert fft_len(na, nb) == N == X.xc_fft_len(na, nb) and X.section_counts(na, nb) == (1, 1)
        assert na + nb - 1 == (N if kind == "fit" else 13 if N == 8192 else N // 2 + 1), (N, kind)
        assert (na, nb) == (7, 7) or (na > nb and 0.75 < nb / na < 0.85)
    assert {na & 1 for _, _, na, _ in cases} == {nb & 1 for _, _, _, nb in cases} == {0, 1}
    (na, nb), (ma, mb) = X.SECTIONED_SHAPES
    assert na + nb - 1 == 2 ** 20 + 1 and fft_len(na, nb) == 2 ** 20
    assert X.section_counts(na, nb) == (2, 2) and na - X.SECTION == nb - X.SECTION == 1       # sections of 2^19 and 1
    assert X.section_counts(ma, mb) == (2, 2) and (ma - X.SECTION, mb - X.SECTION) == (175_713, 1)


def test_signal_kinds():
    """the four kinds differ where it matters to a float32 transform: the narrow band and the tone correlate strongly at every lag"""
    na, nb = 9103, 7282
    norms = {}
    for kind in X.KINDS:
        a, b = X.signal_pair(kind, na, nb)
        assert a.shape == (na,) and b.shape == (nb,) and np.isfinite(a).all() and np.isfinite(b).all()
        norms[kind] = float(np.linalg.norm(X.full_fft(a, b)))
    print("\n||full||_2 by kind: " + ", ".join(f"{k} {v:.2f}" for k, v in norms.items()))
    assert norms["white"] < 2.0 and min(norms["narrow"], norms["tone"], norms["dc"]) > 5.0 * norms["white"]


def test_flat_top_case():
    """the float64 correlation of the flat-topped take drops by less than 1e-6 over three lags on either side of its peak, the peak is
    unique among the lags a +/-2 refinement can reach, and no rival is listed elsewhere"""
    a, b = X.flat_top_case()
    o = X.oracle_delay(a, b)
    near = X.exact_at(a, b, range(o.peak - 3, o.peak + 4))
    drop = float(near[3] - min(near[0], near[6]))
    print(f"\nflat top: peak {o.peak}, delay {o.delay:.4f}, drop over three lags {drop:.3e}, D {o.fm - 2 * o.f0 + o.fp:.3e}, "
          f"4 x delay bound {4 * X.delay_bounds(o.fm, o.f0, o.fp, len(b))[0]:.2e} samples")
    assert 0.0 < drop < 1e-6 and int(np.argmax(near)) == 3
    assert np.all(np.diff(near[:4]) > 100 * X.delta_f(len(b))) and np.all(np.diff(near[3:]) < -100 * X.delta_f(len(b)))
    assert abs(-o.delay - 1234.4) < 1.0                           # b is the later take; the windows pull the peak by half a lag
    top, rivals = X.rivals_of(X.same_fft(a, b))
    assert top == o.peak and len(rivals) == 0


def test_interp_inputs():
    """the np.interp inputs hold the values they exist for, and the oracle treats them as the kernel's comment says"""
    n = 1000
    pos = X.lerp_positions(n, 0.0, 1000)
    sig = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    want = X.lerp_oracle(pos, sig)
    assert np.isnan(pos).sum() == 1 and np.isnan(want).sum() == 1 and (pos == n - 1).any() and (pos > n - 1).sum() == 1
    assert want[pos > n - 1][0] == 0.0 and want[pos == n - 1][0] == sig[-1] and np.all(want[pos < 0] == 0.0)
    assert want[np.signbit(pos) & (pos == 0)][0] == sig[0]                       # -0.0 is inside the signal
    assert (pos == np.floor(pos)).sum() >= 125
    big = (1 << 24) + 1001
    pos = X.lerp_positions(big, big - 1000, 1000)
    assert np.nanmin(pos[pos > 0]) >= big - 1000 > 2 ** 24 and (np.float32(pos[0]) != pos[0] or pos[0] == np.floor(pos[0]))
    from oracle import oracle_np as O
    curves = X.lag_curves()
    lens = {name: len(O.lag_to_positions(c, sr, n)) for name, (c, sr, n) in curves.items()}
    assert lens["cut_at_0"] == 0 and 0 < lens["crosses_midway"] < 24000
    for name in ("two_points", "repeated_time", "crosses_nowhere"):
        c, sr, n = curves[name]
        assert lens[name] == int(np.ceil(n + abs(c[-1, 1] * sr))), name
    assert curves["two_points"][0].shape == (2, 2) and curves["two_points_negative_lag"][0].shape == (2, 2)
    c, sr, n = curves["repeated_time"]
    assert (np.diff(c[:, 0]) == 0).sum() == 1 and float(c[2, 0] * sr).is_integer()
    c, sr, n = curves["x_on_knots"]
    assert all(float(t * sr).is_integer() for t in c[:, 0])


def test_interp_inputs_beside_samples_that_are_not_finite():
    """np.interp on the signals of lerp_nonfinite gives the values written out below, and the bare slope formula -- what a kernel without
    np.interp's x == xp[j] branch and its retry from the right knot computes -- differs from it at every position the inputs exist for"""
    sig, pos = X.lerp_nonfinite()["inf_and_nan"]
    want = X.lerp_oracle(pos, sig)
    table = {0.0: 1.0, 1.0: np.inf, 1.5: np.inf, 2.0: np.inf, 3.0: 2.0, 0.5: np.inf, 2.5: np.inf, 5.0: 3.0, 5.5: 3.5, 6.0: 4.0}
    for x, y in table.items():
        assert np.all(want[pos == x] == y), (x, y, want[pos == x])                 # (pos == 0.0 holds for -0.0 too)
    assert np.signbit(pos[1]) and np.isnan(want[(pos > 3.0) & (pos < 5.0)]).all() and np.isfinite(want[pos >= 5.0]).all()

    def bare(pos, sig):
        i = np.minimum(np.floor(pos).astype(np.int64), len(sig) - 2)
        y0, y1 = sig[i].astype(np.float64), sig[i + 1].astype(np.float64)
        with np.errstate(invalid="ignore"):
            return ((y1 - y0) * (pos - i) + y0).astype(np.float32)
    for name, at in (("inf_and_nan", [0.0, 1.0, 1.5, 2.0, 2.5, 3.0]), ("minus_inf", [0.0, 2.0, 3.0, 3.5, 4.0]), ("signed_zero", [0.0, 2.0, 3.0])):
        sig, pos = X.lerp_nonfinite()[name]
        want, plain = X.lerp_oracle(pos, sig), bare(pos, sig)
        differ = (want.view(np.uint32) != plain.view(np.uint32)) & ~(np.isnan(want) & np.isnan(plain))
        assert set(at) <= set(pos[differ]), (name, pos[differ])


def test_zz_run_time():
    print(f"\ntests/test_xcorr_inputs_cpu.py: {time.perf_counter() - T0:.1f} s since import")
