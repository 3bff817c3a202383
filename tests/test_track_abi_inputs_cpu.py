"""The inputs of tests/test_track_abi_gpu.py, checked without a GPU: every case of tests/track_abi_inputs.py drives the path it is
named for, no comparison rests on a rounding cliff, the correlation statement agrees with oracle_np.xcorr / parabolic, and the two
entry points refuse a row pitch below the row length before they touch a device."""
import ctypes

import numpy as np
import pytest

import track_abi_inputs as T
from oracle import oracle_np as O


# ================================================================================================ piptrack
@pytest.fixture(scope="module")
def pip():
    """case name -> (S32, pitches, mags) of the statement, computed once"""
    out = {}
    for c in T.PIP_CASES:
        S = T.pip_S32(c)
        p, m = T.piptrack_statement(c, S)
        out[c.name] = (S, p, m)
    return out


def test_piptrack_cases_cover_the_stated_shapes():
    cs = T.PIP_CASES
    assert len({c.name for c in cs}) == len(cs)
    assert {c.bins for c in cs} == {2, 3, 63, 64, 65, 129, 257}
    assert {c.frames for c in cs} == {1, 3, 4, 5, 9}
    for bins in (2, 3, 63, 64, 65, 129, 257):
        assert {c.pitch - c.bins for c in cs if c.bins == bins} == {0, 37}, bins
    assert any(c.bins == c.fft_size // 2 + 1 for c in cs) and any(c.bins < c.fft_size // 2 + 1 for c in cs)
    assert any(c.frames % 4 for c in cs) and any(c.frames > 4 and c.frames % 4 for c in cs)          # a partial last workgroup
    assert any(c.fmin < 0 for c in cs) and any(c.fmax > c.sr / 2 for c in cs)
    kinds = {(float(c.scale), float(c.offset)) for c in cs}
    assert (1.0, 0.0) in kinds and any(o == float(np.float32(1e-7)) and s == float(np.float32(np.sqrt(c.fft_size)))
                                       for c in cs for s, o in [(float(c.scale), float(c.offset))])
    for c in cs:
        assert c.sr == 48000 and c.fft_size & (c.fft_size - 1) == 0 and c.mag.dtype == np.float32
        assert c.mag.shape == (c.frames, c.pitch) and np.all(c.mag[:, c.bins:] == T.PAD)
        assert np.all(np.isfinite(c.mag)) and np.all(c.mag[:, :c.bins] < 4)
        # bin frequencies are exact doubles and numpy's rfftfreq returns exactly those
        k = np.arange(c.fft_size // 2 + 1)
        assert np.array_equal(np.fft.rfftfreq(c.fft_size, 1.0 / c.sr), k * c.sr / c.fft_size)
        assert np.array_equal(k * c.sr / c.fft_size * c.fft_size, k * c.sr)


def local_max(S, ref):
    """the oracle's peak pattern before the frequency mask, on (frames, bins)"""
    x = S * (S > ref)
    xp = np.pad(x, ((0, 0), (1, 1)), mode="edge")
    return (x > xp[:, :-2]) & (x >= xp[:, 2:]), x


def test_piptrack_cases_drive_every_branch(pip):
    seen = dict.fromkeys(("plateau", "last_bin", "at_threshold", "on_fmin", "on_fmax", "below_offset", "bin0_max", "zero_column",
                          "raw_neighbours_below"), 0)
    for c in T.PIP_CASES:
        S, p, m = pip[c.name]
        assert S.dtype == p.dtype == m.dtype == np.float32 and p.shape == m.shape == (c.frames, c.bins)
        assert np.array_equal(p != 0, m != 0) and np.all(np.isfinite(p)) and np.all(np.isfinite(m))
        ref = np.float32(c.threshold) * S.max(axis=1, keepdims=True)
        lm, x = local_max(S, ref)
        f = np.arange(c.bins) * c.sr / c.fft_size
        inside = (max(c.fmin, 0.0) <= f) & (f < min(c.fmax, c.sr / 2))
        assert np.array_equal(p != 0, lm & inside[None, :]), c.name          # the pattern, restated; values are the oracle's
        peak = p != 0
        seen["plateau"] += int(np.sum(peak[:, :-1] & (x[:, 1:] == x[:, :-1])))
        seen["last_bin"] += int(np.sum(peak[:, -1]))
        seen["at_threshold"] += int(np.sum((S == ref) & (S > 0) & ~peak & inside[None, :]
                                           & local_max(S, np.float32(0.999) * ref)[0]))
        if c.fmin > 0:
            seen["on_fmin"] += int(np.sum(peak[:, f == c.fmin]))
        seen["on_fmax"] += int(np.sum(lm[:, f == c.fmax] & ~peak[:, f == c.fmax])) if c.fmax < c.sr / 2 else 0
        seen["below_offset"] += int(np.sum(peak & (c.mag[:, :c.bins] < c.offset)))
        seen["bin0_max"] += int(np.sum((S.argmax(axis=1) == 0) & (S.max(axis=1) > 0) & ~peak[:, 0]))
        seen["zero_column"] += int(np.sum(~S.any(axis=1)))
        if c.bins > 2:
            seen["raw_neighbours_below"] += int(np.sum(peak[:, 1:-1] & (S[:, :-2] > 0) & (S[:, :-2] <= ref) & (S[:, 2:] > 0)
                                                       & (S[:, 2:] <= ref)))
        if c.random:
            assert peak.mean() >= 0.05 or c.bins <= 3, (c.name, peak.mean())
    assert all(v > 0 for v in seen.values()), seen
    # the hand-built columns, cell by cell
    S, p, m = pip["hand_on_bins"]
    assert p[0, 10] == T.bin_hz(10.5, 256) and p[0, 11] == 0 and p[0, 31] > 0 and not p[0, 32:34].any()
    assert p[1, 0] == 0 and m[1, 0] == 0 and p[1, 21] > 0   # bin 0 is the maximum and no pitch; the threshold still follows it
    assert not p[2].any() and not m[2].any()
    assert p[3, 20] > 0 and p[3, 30] == 0 and S[3, 30] == np.float32(0.5) * S[3].max()
    assert p[4, 20] != T.bin_hz(20, 256) and p[4, 26] != 0          # the raw neighbours moved the parabola's vertex
    assert p[5, 64] == 0 and p[5, 16] > 0                   # the last bin lies above fmax here
    assert p[6, 5] == 0 and p[6, 8] > 0 and p[6, 40] == 0 and p[6, 45] == 0
    assert p[7, 7] == 0 and p[7, 8] == 0 and p[7, 39] == T.bin_hz(39.5, 256) and p[7, 40] == 0
    assert np.array_equal(np.nonzero(p[8])[0], np.arange(10, 40, 4))
    assert pip["hand_open"][1][5, 64] == 0                  # bins == fft_size / 2 + 1: the last bin is Nyquist and never inside
    _, p, m = pip["hand_below_nyquist_open"]
    assert p[5, 64] == T.bin_hz(64, 1024) and m[5, 64] == 1.0       # the last bin below Nyquist: a pitch, shift 0


def test_piptrack_offset_cases_have_cells_below_the_offset():
    below = [c for c in T.PIP_CASES if c.name.startswith("below_offset")]
    assert len(below) == 2
    for c in below:
        raw = (c.mag[:, :c.bins] - c.offset) * c.scale
        share = float(np.mean(raw < 0))
        assert 0.03 <= share <= 0.09, (c.name, share)
    for c in T.PIP_CASES:
        if not c.name.startswith("below_offset"):
            assert np.all((c.mag[:, :c.bins] - c.offset) * c.scale >= 0), c.name       # get_mag cannot produce a negative S


def test_piptrack_statement_can_see_a_fused_multiply_add(pip):
    """S + fl(0.5 avg shift) and fma(0.5 avg, shift, S) differ in some peaks of these inputs: a kernel that leaves the product
    unrounded cannot pass the bit comparison."""
    differ = cells = 0
    for c in T.PIP_CASES:
        S, p, m = pip[c.name]
        if c.bins < 3:
            continue
        b = (S[:, 2:] - S[:, :-2]) / np.float32(2)
        a = S[:, 2:] + S[:, :-2] - np.float32(2) * S[:, 1:-1]
        with np.errstate(divide="ignore", invalid="ignore"):
            shift = np.where(np.abs(b) < np.abs(a), -b / a, np.float32(0))
        assert shift.dtype == np.float32
        fused = (S[:, 1:-1].astype(np.float64) + (np.float32(0.5) * b).astype(np.float64) * shift.astype(np.float64)).astype(np.float32)
        peak = p[:, 1:-1] != 0
        cells += int(peak.sum())
        differ += int(np.sum(peak & (fused != m[:, 1:-1])))
    assert differ > 0 and cells > 500, (differ, cells)


# ================================================================================================ correlation
def test_correlation_cases_cover_the_stated_sizes():
    cs = T.CORR_CASES
    sizes = {(c.nb, c.n) for c in cs}
    assert {(3, 12), (5, 20), (17, 68), (65, 260), (129, 516)} <= sizes
    assert {c.count for c in cs if c.nb == 3} == {1, 2}
    assert any(c.NL > 0 and c.NU > c.bins and c.nb == c.bins - c.NL and c.M.shape == (c.n, c.nb) for c in cs)
    assert any(c.count < c.n_frames and np.all(c.mag[c.count:] == T.PAD) for c in cs)
    for c in cs + T.CORR_REALISTIC:
        assert c.n == 4 * (c.NU - c.NL) and c.M.shape == (c.n, c.nb) and c.wind.shape == (c.n,) and c.nb >= 3
        assert c.mag.dtype == np.float32 and c.mag.shape == (c.n_frames, c.bins)
    for c in cs:
        assert np.all(c.wind == 1) and np.all((c.M == 0) | (c.M == 1)) and np.all(c.M.sum(axis=1) <= 1)
        band = c.mag[:c.count, c.NL:c.NL + c.nb]
        assert np.all(band == np.rint(band)) and np.all(np.abs(band) < 16)
        R = T.corr_rows(c)
        assert np.all(R == np.rint(R)) and np.all(R[-1] == 1)
        # every un-normalised sum is an integer far below 2^53: exact in any order of summation
        assert np.sum(np.abs(R), axis=1).max() ** 2 < 2.0 ** 40
    assert {c.nb for c in T.CORR_REALISTIC} == {7, 33}
    for c in T.CORR_REALISTIC:
        assert np.array_equal(c.wind, np.hanning(c.n)) and np.all(np.isfinite(c.M))


def test_correlation_cases_drive_the_named_paths():
    kinds = set()
    for c in T.CORR_CASES + T.CORR_REALISTIC:
        R = T.corr_rows(c)
        same = T.corr_same(c, R)
        for i in range(c.count):
            s = same[i]
            sp = c.special.get(i, ("plain",))
            kinds.add(sp[0])
            if sp[0] == "nan":
                assert np.all(np.isnan(s)) and T.first_argmax(s) == 0, (c.name, i)
                continue
            assert np.all(np.isfinite(s)), (c.name, i)
            peak = T.first_argmax(s)
            top = s[peak]
            at_top = np.nonzero(s == top)[0]                # bit-equal maxima
            if sp[0] == "tie":
                assert peak == sp[1] and tuple(at_top[1:]) == sp[2] and len(at_top) >= 2, (c.name, at_top)
                continue
            if sp[0] == "tie_below_max":
                assert peak == sp[1] and len(at_top) == 1, (c.name, at_top)
                rest = np.where(np.abs(np.arange(c.n) - peak) > 2, s, -np.inf)      # beside the maximum's own flanks
                second = np.nonzero(rest == rest.max())[0]
                assert tuple(second) == sp[2] and second.min() >= 192 and peak < 192, (c.name, second)   # the tie sits in the last wave
            # not a tie: a single maximum, and every lag more than one away lies at least 1e-6 of its height below it
            assert len(at_top) == 1 and top > 0, (c.name, i, at_top)
            far = np.abs(np.arange(c.n) - peak) > 1
            if sp[0] == "lag0":
                far &= np.arange(c.n) != c.n - 1            # the wrapped neighbour
            assert top - s[far].max() >= 1e-6 * top, (c.name, i)
            if sp[0] == "lag0":
                assert peak == 0 and s[c.n - 1] != s[1] and s[c.n - 1] != 0
                assert np.count_nonzero(R[i]) >= 3 and np.count_nonzero(R[i + 1]) >= 3
                wrapped = O.parabolic(s, 0)[0]
                for other in (s[1], 0.0, s[0]):             # a mirrored, a zero or a clamped neighbour would give another vertex
                    assert abs(O.parabolic(np.concatenate((s, [other])), 0)[0] - wrapped) > 1e-3
            elif sp[0] == "last_lag":
                assert peak == c.n - 1
                with pytest.raises(IndexError):
                    O.parabolic(s, peak)
            else:
                assert 0 < peak < c.n - 1, (c.name, i, peak)
            if sp[0] != "last_lag":
                # the statement and the oracle's own xcorr / parabolic agree on the refined peak
                mine = O.parabolic(s, peak)[0]
                assert abs(mine - T.corr_oracle_refined(c, i, R)) <= 1e-12, (c.name, i)
    assert kinds == {"plain", "nan", "tie", "tie_below_max", "lag0", "last_lag"}


def test_correlation_statement_results():
    for c in T.CORR_CASES + T.CORR_REALISTIC:
        if any(sp[0] == "last_lag" for sp in c.special.values()):
            with pytest.raises(IndexError):
                T.corr_statement(c)
            continue
        st = T.corr_statement(c)
        nan_pairs = sorted(i for i, sp in c.special.items() if sp[0] == "nan")
        assert np.array_equal(np.nonzero(np.isnan(st["changes"]))[0], nan_pairs), c.name
        if nan_pairs:                                       # silent frame k: pairs k-1 and k; the running sum is NaN from k-1 on
            k = nan_pairs[0]
            assert nan_pairs == [2, 3] and np.all(np.isfinite(st["cum"][:k])) and np.all(np.isnan(st["cum"][k:]))
        assert np.nanmax(np.abs(st["cum"])) < 900           # exp2 of the running sum stays a normal double
    c = next(c for c in T.CORR_CASES if c.name == "sizes_nb3_n12_c1")
    assert c.count == 1 and T.corr_statement(c)["peaks"][0] == c.n // 2        # the only pair is with the all-ones frame
    moved = [c.name for c in T.CORR_REALISTIC if np.all(np.abs(T.corr_statement(c)["changes"][:-1]) > 1e-3)]
    assert len(moved) == 2                                  # the realistic bumps really move between frames


# ================================================================================================ zero crossings
def test_zero_crossing_vectors_put_every_pair_on_every_seam():
    seq = T.ZC_SEQUENCE
    L = len(seq)
    assert L == 11 and np.signbit(seq[1]) and not np.signbit(seq[0]) and seq[2] == 5e-324 and seq[2] > 0 and seq[3] < 0
    for seam in (255, 511, 1023, 2047):
        pairs = {tuple(x[seam:seam + 2].view(np.uint64).tolist()) for x in T.ZC_VECTORS.values() if len(x) > seam + 1}
        assert pairs >= {tuple(np.roll(seq, -j)[:2].view(np.uint64).tolist()) for j in range(L)}, seam
    x = T.ZC_VECTORS["rot0_n11"]
    # +0 -0 tiny -tiny nan 1 nan -1 inf -inf 0: NaN, zeros and negatives are "not positive"
    assert T.zc_statement(x).tolist() == [1, 2, 4, 5, 7, 8]
    assert np.array_equal(T.zc_statement(x), O.zero_crossings(x))
    assert all(len(T.zc_statement(x)) >= 1 for x in T.ZC_VECTORS.values() if len(x) > 2)
    assert len(T.zc_statement(T.ZC_VECTORS["rot0_n2"])) == 0          # +0 -0: the count kernels run and find nothing


# ================================================================================================ argument checks
def test_row_pitch_below_the_row_length_is_refused_before_any_device_call():
    """PAR_ERR_ARG without a GPU in sight: the checks run before hipSetDevice (a device call here would answer PAR_ERR_HIP)"""
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(8)
    for pitch in (1, 64):
        rc = L.par_piptrack_f32(0, p, 4, 65, pitch, 1.0, 0.0, 128, 48000.0, 0.0, 24000.0, 0.1, p, p, None)
        assert rc == 1 and "par_piptrack_f32: mag_pitch < bins" in _lib.last_error(), (rc, _lib.last_error())
        rc = L.par_track_corr_f64(0, p, 4, 65, pitch, 2, 19, 3, p, p, 68, 68.0, 0.0, p, p, p, None)
        assert rc == 1 and "par_track_corr_f64: mag_pitch < bins" in _lib.last_error(), (rc, _lib.last_error())
    # the other argument checks of the two entry points, equally host-only
    assert L.par_piptrack_f32(0, None, 4, 65, 0, 1.0, 0.0, 128, 48000.0, 0.0, 24000.0, 0.1, p, p, None) == 1
    assert "par_piptrack_f32: null pointer" in _lib.last_error()
    assert L.par_piptrack_f32(0, p, 4, 1, 0, 1.0, 0.0, 128, 48000.0, 0.0, 24000.0, 0.1, p, p, None) == 1
    assert "par_piptrack_f32: bad sizes" in _lib.last_error()
    assert L.par_piptrack_f32(0, p, 0, 65, 0, 1.0, 0.0, 128, 48000.0, 0.0, 24000.0, 0.1, p, p, None) == 0        # no frames: nothing to do
    assert L.par_track_corr_f64(0, p, 4, 65, 0, 2, 19, 3, p, p, 68, 68.0, 0.0, None, p, p, None) == 1
    assert "par_track_corr_f64: null pointer" in _lib.last_error()
    for NL, NU, n, count in ((2, 4, 8, 3), (-1, 16, 68, 3), (2, 19, 64, 3), (2, 19, 68, 5), (63, 80, 68, 3)):      # nb < 3, NL < 0, n, count
        assert L.par_track_corr_f64(0, p, 4, 65, 0, NL, NU, count, p, p, n, 1.0, 0.0, p, p, p, None) == 1, (NL, NU, n, count)
        assert "par_track_corr_f64: bad band / grid" in _lib.last_error()
    cnt = ctypes.c_int64(5)
    assert L.par_zero_crossings_f64(0, None, 10, p, None, 0, ctypes.byref(cnt), None) == 1
    for n in (0, 1):                                        # nothing to compare: count 0 without a device call
        cnt.value = 5
        assert L.par_zero_crossings_f64(0, p, n, p, None, 0, ctypes.byref(cnt), None) == 0 and cnt.value == 0
    assert L.par_track_corr_work_len(6, 68) == 7 * 68 + 6 and L.par_zero_crossings_work_len(2100) == 4
