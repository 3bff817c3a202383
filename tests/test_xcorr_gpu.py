"""The tape-sync path kernel by kernel: par_xcorr_f64 / par_find_delay_f64 (the X2 block of csrc/stft.hip) through correlation.py and
pipeline.correlate_sources, and the two np.interp kernels of csrc/lag.hip, against the float64 oracles of tests/xcorr_inputs.py --
where the end-to-end tests of test_hip_parity.py do not reach: every transform size from 2^13 to 2^20 at its exact fit and at its
smallest member, the smallest sectioned shape (sections of 2^19 and 1 sample), peaks on lags 0, 1, 2, na-3 and na-2, nb > na and
nb << na, 1 to 63 rival peaks and the 64-rival plateau, a top so flat that the float32 transform cannot place it, and np.interp bit
for bit past position 2^24 and on a strided channel.

Bounds: the float32 transform's error is MEASURED here (test 1) and asserted against the one constant that depends on it,
kXcRivalTol (twice the error must not exceed it, or a rival could go unlisted); everything find_delay returns is held to
xcorr_inputs.delay_bounds, derived from the rounding of a float64 dot product, at 4 x; the np.interp kernels to equality.
tests/test_xcorr_inputs_cpu.py proves the preconditions of every input.  pytest -s prints the measured figures (NOTES.md, Correlation)."""
import logging

import numpy as np
import pytest
import scipy.signal

import xcorr_inputs as X

pytestmark = pytest.mark.gpu

RIVAL_TOL = 4.0e-6          # kXcRivalTol of csrc/stft.hip; its meaning: include/par_hip.h, par_find_delay_f64
MODE_BOUND = RIVAL_TOL / 2  # the ceiling test 1 puts on the transform's error in every regime: not a device figure
FFT64_BOUND = 1e-10         # float64 FFT against fsum: rounding ~ 2^-53 log2(N) on values <= 1 is ~1e-14; 1e-10 is still 1e-4 of what
                            # is measured against it
SAFETY = 4.0                # the tests use 4 x delay_bounds


@pytest.fixture(scope="module")
def C():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pyaudiorestoration_amd import correlation
    return correlation


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- 1. transform error per regime, tied to the listing tolerance ------------------------------------------------------------------
def _transform_errors(C, label, shapes, check_fft64):
    rows, rng = [], np.random.default_rng(len(label))
    for na, nb in shapes:
        for kind in X.KINDS:
            a, b = X.signal_pair(kind, na, nb)
            want = X.full_fft(a, b)
            if check_fft64 and kind == "narrow":          # the float64 side itself, once per class, on the kind with the largest ||full||
                lags = rng.integers(0, na + nb - 1, 50)
                e64 = float(np.max(np.abs(want[lags] - X.exact_at(a, b, lags, full=True))))
                print(f"\n{label}: float64 FFT against fsum at 50 lags: {e64:.2e}", end="")
                assert e64 <= FFT64_BOUND
                check_fft64 = False
            got = C.xcorr(a, b, "full")
            assert got.shape == want.shape and got.dtype == np.float64
            rows.append((na, nb, kind, float(np.max(np.abs(got - want)))))
    for na, nb, kind, err in rows:
        print(f"\n{label:>9s} {na:7d} x {nb:7d} {kind:7s} err {err:.3e}  2 err / kXcRivalTol {2 * err / RIVAL_TOL:.3f}", end="")
    for na, nb, kind, err in rows:
        assert 2.0 * err <= RIVAL_TOL, (label, na, nb, kind, err)


@pytest.mark.parametrize("N", [1 << k for k in range(13, 21)])
def test_transform_error_single(C, N):
    """max |xcorr(a, b, 'full') - float64| for the exact-fit and the smallest shape of transform size N, four signal kinds:
    2 x error <= kXcRivalTol"""
    shapes = [(na, nb) for n, _, na, nb in X.size_classes() if n == N]
    assert len(shapes) == 2
    _transform_errors(C, f"N=2^{N.bit_length() - 1}", shapes, True)


@pytest.mark.parametrize("na,nb", X.SECTIONED_SHAPES)
def test_transform_error_sectioned(C, na, nb):
    """the same for the sectioned form: sections of 2^19 and 1 sample, and 2 x 2 pairs with unequal tails"""
    _transform_errors(C, "sectioned", [(na, nb)], (na, nb) == X.SECTIONED_SHAPES[0])


@pytest.mark.parametrize("ga,gb", [(1.0, 1e-4), (1e-4, 1.0), (3e4, 1e-3)])
def test_transform_error_unequal_levels(C, ga, gb):
    """the normalised correlation does not depend on either take's level, and neither may its error: a + i b goes through ONE
    float32 transform, so the takes are packed normalised (packed raw, the quieter take carried the louder one's rounding: the
    7 x 7 narrow-band pair of test 1, whose takes differ 63 dB in level, measured 2.1e-5).  One single-transform and one sectioned
    shape, white noise, gains 80 dB and 150 dB apart."""
    for na, nb in ((36411, 29127), X.SECTIONED_SHAPES[0]):
        a, b = X.signal_pair("white", na, nb)
        err = float(np.max(np.abs(C.xcorr(ga * a, gb * b, "full") - X.full_fft(a, b))))
        print(f"\ngains {ga:g} / {gb:g} {na:7d} x {nb:7d} err {err:.3e}  2 err / kXcRivalTol {2 * err / RIVAL_TOL:.3f}", end="")
        assert 2.0 * err <= RIVAL_TOL, (ga, gb, na, nb, err)


# ---- 2. xcorr modes at the class edges ---------------------------------------------------------------------------------------------
def _mode_shapes():
    cls = X.size_classes()
    mins = [(na, nb) for _, kind, na, nb in cls if kind == "min"][:2]
    fits = [(na, nb) for _, kind, na, nb in cls if kind == "fit"]
    return mins + [fits[0], fits[-1]] + [X.SECTIONED_SHAPES[0]]


@pytest.mark.parametrize("na,nb", _mode_shapes())
def test_xcorr_modes_at_class_edges(C, na, nb):
    """'full', 'same' and 'valid' against scipy's float64 correlation of the normalised inputs, in both argument orders (nb > na has
    no 'valid' here, like the reference's use).  A wrong wrap or section offset is an O(1) error."""
    for u, v in ((na, nb), (nb, na)):
        a, b = X.signal_pair("white", u, v)
        an, bn = X.normalised(a), X.normalised(b)
        for mode in ("full", "same") + (("valid",) if u >= v else ()):
            want = scipy.signal.correlate(an, bn, mode=mode, method="fft")
            got = C.xcorr(a, b, mode)
            assert got.shape == want.shape, (u, v, mode)
            err = float(np.max(np.abs(got - want)))
            print(f"\n{u:7d} x {v:7d} {mode:5s} err {err:.3e}", end="")
            assert err <= MODE_BOUND, (u, v, mode, err)


# ---- 3. edge lags ------------------------------------------------------------------------------------------------------------------
def _held(got, o, nb):
    """|delay - oracle| and |corr - oracle| as multiples of the derived bounds; the caller asserts <= SAFETY"""
    bd, bc = X.delay_bounds(o.fm, o.f0, o.fp, nb)
    return abs(got[0] - o.delay) / bd, abs(got[1] - o.corr) / bc


@pytest.mark.parametrize("na,nb", X.EDGE_SHAPES)
def test_find_delay_edge_lags(C, na, nb):
    """peaks on lag 0 (f[-1] wraps to the last lag, like numpy), 1, 2, na-3, na-2 under both ignore_phase settings: the oracle's
    find_delay and the fsum oracle, within 4 x delay_bounds; a peak on na-1 is the reference's IndexError"""
    from oracle import oracle_np as O
    worst = (0.0, 0.0)
    for want in X.edge_peaks(na):
        for ign in (False, True):
            a, b = X.edge_case(na, nb, want)
            o = X.oracle_delay(a, b, ign)
            ref = O.find_delay(a.copy(), b.copy(), ignore_phase=ign)
            got = C.find_delay(a.copy(), b.copy(), ignore_phase=ign)
            assert o.peak == want and round(got[0] + na // 2) == want, (want, ign, got)
            r = _held(got, o, nb)
            bd, bc = X.delay_bounds(o.fm, o.f0, o.fp, nb)
            rr = (abs(got[0] - ref[0]) / bd, abs(got[1] - ref[1]) / bc)
            worst = (max(worst[0], r[0], rr[0]), max(worst[1], r[1], rr[1]))
            assert max(r) <= SAFETY and max(rr) <= SAFETY, (na, nb, want, ign, got, o, ref, r, rr)
    print(f"\nedge lags {na} x {nb}: worst delay error {worst[0]:.2e}, corr error {worst[1]:.2e} of the derived bounds", end="")
    a, b = X.edge_case(na, nb, na - 1)
    with pytest.raises(IndexError):
        O.find_delay(a.copy(), b.copy())
    with pytest.raises(IndexError):
        C.find_delay(a.copy(), b.copy())


def test_find_delay_edge_lags_sectioned(C):
    """the same where the peak stage scans the float64 'full' array of 2 x 2 section pairs with 1024 threads, which no batch reaches:
    peaks on lag 0 (f[-1], the eighth exact value) and na-2 under both ignore_phase settings, within 4 x delay_bounds of the fsum
    oracle (about 1.07e-9 samples and 5.8e-10 corr: tests/test_xcorr_inputs_cpu.py); a peak on na-1 is the reference's IndexError"""
    na, nb = X.SECTIONED_SHAPES[0]
    for want in X.sectioned_edge_peaks():
        a, b = X.edge_case(na, nb, want)
        for ign in (False, True):
            o = X.oracle_delay(a, b, ign)
            got = C.find_delay(a.copy(), b.copy(), ignore_phase=ign)
            r = _held(got, o, nb)
            print(f"\nsectioned edge lag {want} ign {ign}: delay error {r[0]:.2e}, corr error {r[1]:.2e} of the derived bounds", end="")
            assert o.peak == want and round(got[0] + na // 2) == want, (want, ign, got)
            assert max(r) <= SAFETY, (want, ign, got, o, r)
    a, b = X.edge_case(na, nb, na - 1)
    with pytest.raises(IndexError):
        C.find_delay(a.copy(), b.copy())


@pytest.mark.parametrize("na,nb", X.SCRATCH_SHAPES)
def test_single_calls_stay_inside_their_scratch(C, na, nb):
    """par_find_delay_f64 and par_xcorr_f64 at the ABI, on a scratch of exactly par_xcorr_scratch_bytes(na, nb) bytes followed by 256
    sentinel bytes: the row record and the results of the delay search live in the spare room behind
    the lags, and must not leave it.  The sentinels (behind `full` too) keep their bits, and a second call on the used scratch gives
    the same bits."""
    import ctypes
    import torch
    from pyaudiorestoration_amd import _dev, _lib
    L = _lib.lib()
    a, b = X.signal_pair("white", na, nb)
    a_t, b_t = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    nbytes, guard, n_full = int(L.par_xcorr_scratch_bytes(na, nb)), 256, na + nb - 1
    scratch = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    full = torch.full((n_full + 32,), -7.25e11, dtype=torch.float64, device="cuda")
    runs = []
    for _ in range(2):
        delay, corr = ctypes.c_double(0.0), ctypes.c_double(0.0)
        for ign in (0, 1):
            _lib.check(L.par_find_delay_f64(0, _dev.ptr(a_t), na, _dev.ptr(b_t), nb, ign, _dev.ptr(scratch), nbytes, ctypes.byref(delay),
                                            ctypes.byref(corr), _dev.stream_ptr(0)))
        _lib.check(L.par_xcorr_f64(0, _dev.ptr(a_t), na, _dev.ptr(b_t), nb, _dev.ptr(scratch), nbytes, _dev.ptr(full), _dev.stream_ptr(0)))
        torch.cuda.synchronize()
        f = full.cpu().numpy()
        assert np.all(scratch[nbytes:].cpu().numpy() == 0xA5) and np.all(f[n_full:] == -7.25e11)
        assert np.isfinite(delay.value) and np.isfinite(corr.value) and np.all(np.isfinite(f[:n_full]))
        runs.append((bits(np.array([delay.value, corr.value])), bits(f)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    o = X.oracle_delay(a, b, True)                                                   # the last call ignored the phase
    assert max(_held((delay.value, corr.value), o, nb)) <= SAFETY, (delay.value, corr.value, o)


def test_correlate_sources_device_tensors_of_unequal_length(C):
    """pytapesynch_gui.py:108-133 hands find_delay whatever get_signal_around returned: under match_speed the source window is
    t_width / speed long and resampled, so len(src) != len(ref) is ACCEPTED there, never checked -- and so it is here.  Device
    tensors in, band-passed and correlated in HBM, the caller's tensors untouched.  The filter is K_sosfiltfilt's, so the bound is
    that flow's own (test_hip_parity.py::test_correlate_sources_flow), not delay_bounds."""
    import torch
    from oracle import oracle_np as O
    from pyaudiorestoration_amd import pipeline
    sr, na, nb = 48000, 24000, 22999
    rng = np.random.default_rng(12)
    base = np.convolve(rng.standard_normal(na + 400), np.hanning(9) / 4, mode="same")
    ref = base[200:200 + na].copy()
    src = (0.8 * np.interp(np.arange(na) + 200 - 37.3, np.arange(len(base)), base) + 0.01 * rng.standard_normal(na))[:nb]
    ref_t, src_t = torch.from_numpy(ref).cuda(), torch.from_numpy(src).cuda()
    for window_name, ign in ((None, False), ("hann", True)):
        want_d, want_c = O.find_delay(O.butter_bandpass_filter(ref.copy(), 300.0, 6000.0, sr, order=3),
                                      O.butter_bandpass_filter(src.copy(), 300.0, 6000.0, sr, order=3), ignore_phase=ign,
                                      window_name=window_name)
        got_d, got_c = pipeline.correlate_sources(ref_t, src_t, sr, 300.0, 6000.0, ign, window_name)
        assert abs(got_d * sr - want_d) < 1e-5 and abs(got_c - want_c) < 1e-8, (window_name, got_d * sr, want_d, got_c, want_c)
        assert np.array_equal(ref_t.cpu().numpy(), ref) and np.array_equal(src_t.cpu().numpy(), src)
    assert abs(abs(want_d) - 37.3 - (na - nb) / 2) < 1.0                    # 'same' centres on the longer take


# ---- 4. rivals ---------------------------------------------------------------------------------------------------------------------
def _rival(C, a, b, lags, loud, ign=False):
    o = X.oracle_delay(a, b, ign)
    assert o.peak == lags[loud]
    got = C.find_delay(a.copy(), b.copy(), ignore_phase=ign)
    r = _held(got, o, len(b))
    assert round(got[0] + len(a) // 2) == lags[loud], (loud, got, o)                 # names the louder copy
    assert max(r) <= SAFETY, (loud, got, o, r)
    return r


@pytest.mark.parametrize("K", X.RIVAL_KS)
def test_find_delay_rivals(C, K):
    """K copies, one 3e-7 louder, first, middle and last: K - 1 rivals are listed (63 fill the kXcCand slots with the top) and the exact
    values pick the louder copy although the float32 transform cannot"""
    for loud in X.rival_positions(K):
        a, b, lags = X.rival_case(K, loud)
        r = _rival(C, a, b, lags, loud)
        print(f"\nK = {K:2d}, louder copy {loud:2d}: delay error {r[0]:.2e}, corr error {r[1]:.2e} of the derived bounds", end="")


def test_find_delay_rival_variants(C):
    """an exact tie goes to the lower lag (np.argmax); an inverted louder copy wins under ignore_phase"""
    a, b, lags = X.rival_case(2, 1, scale=1.0)
    _rival(C, a, b, lags, 0)
    a, b, lags = X.rival_case(2, 1, scale=-(1.0 + X.LOUDER))
    _rival(C, a, b, lags, 1, ign=True)
    _rival(C, a, b, lags, 0, ign=False)


def test_find_delay_plateau_is_a_stated_limit(C):
    """65 copies: 64 rivals do not fit the kXcCand slots beside the top, the call takes them for a plateau and the transform's own top
    stands (include/par_hip.h).  The one statement here that is weaker than equality with the reference: the call succeeds and lands
    ON one of the 65 copies; which one is the float32 transform's choice."""
    a, b, lags = X.rival_case(65, 40)
    got = C.find_delay(a.copy(), b.copy())
    assert np.min(np.abs(got[0] + len(a) // 2 - lags)) <= 0.5, got


def test_find_delay_rival_in_sectioned_regime(C):
    """the K = 2 case through 2 x 2 section pairs, the rival 400 000 lags away"""
    a, b, lags = X.sectioned_rival_case()
    r = _rival(C, a, b, lags, 1)
    print(f"\nsectioned pair: delay error {r[0]:.2e}, corr error {r[1]:.2e} of the derived bounds", end="")


# ---- 5. off-by-lag -----------------------------------------------------------------------------------------------------------------
def test_find_delay_flat_top(C, caplog):
    """the correlation drops by less than 1e-6 over three lags (test_xcorr_inputs_cpu.py records it), so the float32 top may sit beside
    the exact one: the exact re-evaluation must still return the oracle's integer peak and, within delay_bounds, its delay.  |D| is
    ~1e-7 here, so the delay bound is loose (about 2e-3 samples at 1 x) -- the integer peak is the sharp statement."""
    a, b = X.flat_top_case()
    o = X.oracle_delay(a, b)
    with caplog.at_level(logging.DEBUG):
        got = C.find_delay(a.copy(), b.copy())
    i_peak = [float(r.getMessage().split()[1]) for r in caplog.records if r.getMessage().startswith("i_peak ")]
    bd, bc = X.delay_bounds(o.fm, o.f0, o.fp, len(b))
    print(f"\nflat top: oracle peak {o.peak} delay {o.delay:.6f}; device i_peak {i_peak} delay {got[0]:.6f}; bounds (1 x) {bd:.2e} samples, "
          f"{bc:.2e}; errors {abs(got[0] - o.delay) / bd:.2e}, {abs(got[1] - o.corr) / bc:.2e} of them", end="")
    assert len(i_peak) == 1 and round(i_peak[0]) == o.peak, (i_peak, o)
    assert max(_held(got, o, len(b))) <= SAFETY, (got, o)


# ---- 6. the np.interp kernels, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lo", [(1000, 0.0), ((1 << 24) + 1001, float((1 << 24) + 1))])
def test_linear_resample_equals_np_interp(C, n, lo):
    """k_lerp restates np.interp operation by operation without contraction: equal as uint32, on random, integer, n-1, just above n-1,
    negative, -0.0 and NaN positions -- also where a float32 position could not tell two samples apart"""
    import torch
    from pyaudiorestoration_amd import resampling
    sig = np.random.default_rng(n).standard_normal(n, dtype=np.float32)
    pos = X.lerp_positions(n, lo, 1000)
    want = X.lerp_oracle(pos, sig)
    got = resampling.linear_resample_dev(torch.from_numpy(pos).cuda(), torch.from_numpy(sig).cuda()).cpu().numpy()
    diff = np.nonzero(bits(got) != bits(want))[0]
    assert got.dtype == np.float32 and len(diff) == 0, (diff[:5], pos[diff[:5]], got[diff[:5]], want[diff[:5]])


@pytest.mark.parametrize("name", sorted(X.lerp_nonfinite()))
def test_linear_resample_beside_samples_that_are_not_finite(C, name):
    """np.interp's two branches beside the slope formula: x == xp[j] returns fp[j] (slope * 0 would make NaN of an inf neighbour, and
    +0.0 of a sample that is -0.0), and a NaN result is tried again from the right knot -- equal as uint32, a NaN's payload aside"""
    import torch
    from pyaudiorestoration_amd import resampling
    sig, pos = X.lerp_nonfinite()[name]
    want = X.lerp_oracle(pos, sig)
    got = resampling.linear_resample_dev(torch.from_numpy(pos).cuda(), torch.from_numpy(sig).cuda()).cpu().numpy()
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert got.dtype == np.float32 and same.all(), (pos[~same], got[~same], want[~same])


def test_linear_resample_strided_channel_between_sentinels(C):
    """channel 1 of an interleaved stereo buffer into channel 1 of an interleaved output: the other channel's cells and the cells
    around the output keep their sentinel bit for bit, and the poisoned input channel is never read into a result"""
    import torch
    from pyaudiorestoration_amd import resampling
    n, m, guard = 1000, 777, 64
    rng = np.random.default_rng(5)
    sig = rng.standard_normal(n, dtype=np.float32)
    inter = np.full(2 * n, 1e30, np.float32)
    inter[1::2] = sig
    pos = X.lerp_positions(n, 0.0, m)
    out = np.full(2 * m + 2 * guard, -7.25, np.float32)
    out_t, in_t = torch.from_numpy(out.copy()).cuda(), torch.from_numpy(inter).cuda()
    resampling.linear_resample_dev(torch.from_numpy(pos).cuda(), in_t[1:], out_t[guard + 1:], sig_stride=2, len_in=n, out_stride=2)
    now = out_t.cpu().numpy()
    body = now[guard:guard + 2 * m]
    assert np.array_equal(bits(body[1::2]), bits(X.lerp_oracle(pos, sig)))
    assert np.array_equal(bits(body[0::2]), bits(out[:m])) and np.array_equal(bits(now[:guard]), bits(out[:guard]))
    assert np.array_equal(bits(now[guard + 2 * m:]), bits(out[:guard]))


@pytest.mark.parametrize("name", sorted(X.lag_curves()))
def test_lag_to_pos_equals_np_interp(C, name):
    """k_lag_pos against the oracle's np.interp + cut + clip, equal as uint64 and in length: two-point curves, a repeated sample time,
    the cut at output 0, no cut, a cut midway, and outputs that land exactly on knots"""
    from oracle import oracle_np as O
    from pyaudiorestoration_amd import resampling
    curve, sr, n = X.lag_curves()[name]
    want = O.lag_to_positions(curve, sr, n)
    got = resampling.lag_to_pos_dev(curve, sr, n).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float64, (name, got.shape, want.shape)
    diff = np.nonzero(bits(got) != bits(want))[0]
    assert len(diff) == 0, (name, diff[:5], got[diff[:5]], want[diff[:5]])
