"""par_find_delay_sect_f64 on the GPU: the batched, sectioned delay search against the float64 oracles of tests/xcorr_inputs.py
(4 x delay_bounds, the existing margin), bit for bit against the single call par_find_delay_f64, and its 'same' span against
scipy's float64 correlation -- twice the worst lag error must stay below kXcRivalTol, which is the precondition of the
bit-for-bit claim.  S = 4096 (section_log2 12) unless stated, so that every section path is reached with rows of a few thousand
samples.  pytest -s prints the measured figures."""
import functools
import math

import numpy as np
import pytest

import azimuth_inputs as A
import xcorr_inputs as X

pytestmark = pytest.mark.gpu
SENTINEL = -7.25e11
S = 4096
SHAPES = ((3000, 3000), (S + 1, S + 1), (3 * S + 5, 2 * S - 1), (2 * S - 1, 3 * S + 5), (4 * S, 4 * S), (4 * S + 1, 4 * S))


@pytest.fixture(scope="module")
def C():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pyaudiorestoration_amd import correlation
    return correlation


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def pitched(rows, extra):
    import torch
    W, n = rows.shape
    buf = torch.full((W, n + extra), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :n] = torch.tensor(rows, dtype=torch.float64, device="cuda")
    return buf[:, :n], buf


def run_sect(a, b, ign=False, sec=12, scratch_bytes=None, want_same=True):
    """the ABI call itself on pitched rows, every output between sentinel cells -> (delay, corr, status, norms, same)"""
    import torch
    from pyaudiorestoration_amd import _dev, _lib
    L = _lib.lib()
    W, na = a.shape
    nb = b.shape[1]
    a_v, a_buf = pitched(a, 5)
    b_v, b_buf = pitched(b, 3)
    before = (a_buf.clone(), b_buf.clone())
    out = torch.full((2, W + 2), SENTINEL, dtype=torch.float64, device="cuda")
    st = torch.full((W + 2,), -77, dtype=torch.int32, device="cuda")
    nr = torch.full((W + 2, 2), SENTINEL, dtype=torch.float64, device="cuda")
    sm = torch.full((W + 2, na + 7), SENTINEL, dtype=torch.float64, device="cuda")
    nbytes = int(L.par_find_delay_sect_scratch_bytes(na, nb, W, sec)) if scratch_bytes is None else int(scratch_bytes)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(L.par_find_delay_sect_f64(0, _dev.ptr(a_v), a_buf.stride(0), na, _dev.ptr(b_v), b_buf.stride(0), nb, W, sec, int(ign),
                                         _dev.ptr(scratch), nbytes, _dev.ptr(out[0, 1:]), _dev.ptr(out[1, 1:]), _dev.ptr(st[1:]),
                                         _dev.ptr(nr[1:]), _dev.ptr(sm[1:]) if want_same else None, sm.stride(0), _dev.stream_ptr(0)))
    torch.cuda.synchronize()
    o, s, n, m = out.cpu().numpy(), st.cpu().numpy(), nr.cpu().numpy(), sm.cpu().numpy()
    assert np.all(o[:, 0] == SENTINEL) and np.all(o[:, -1] == SENTINEL) and s[0] == s[-1] == -77
    assert np.all(n[0] == SENTINEL) and np.all(n[-1] == SENTINEL) and np.all(m[0] == SENTINEL) and np.all(m[-1] == SENTINEL)
    assert np.all(m[:, na:] == SENTINEL) and (want_same or np.all(m == SENTINEL))
    for buf, was in zip((a_buf, b_buf), before):                        # the rows are only read, the gaps stay NaN
        assert np.array_equal(buf.cpu().numpy().view(np.uint64), was.cpu().numpy().view(np.uint64))
    return o[0, 1:-1], o[1, 1:-1], s[1:-1], n[1:-1], m[1:-1, :na]


def single(C, a, b, ign=False):
    """correlation.find_delay (par_find_delay_f64) row by row; a peak on the last lag -> NaN, status 1"""
    d, c, s = np.empty(len(a)), np.empty(len(a)), np.zeros(len(a), dtype=np.int32)
    for w in range(len(a)):
        try:
            d[w], c[w] = C.find_delay(a[w].copy(), b[w].copy(), ignore_phase=ign)
        except IndexError:
            d[w], c[w], s[w] = np.nan, np.nan, 1
    return d, c, s


def check_oracle(a, b, d, c, ign=False):
    worst = 0.0
    for w in range(len(a)):
        o = X.oracle_delay(a[w], b[w], ign)
        bd, bc = X.delay_bounds(o.fm, o.f0, o.fp, b.shape[1])
        r = max(abs(d[w] - o.delay) / bd, abs(c[w] - o.corr) / bc)
        assert r <= A.SAFETY, (a.shape, b.shape, w, d[w], c[w], o, r)
        worst = max(worst, r)
    return worst


@functools.lru_cache(maxsize=None)
def rows_of(na, nb):
    a, b = A.batch_rows(na, nb, 3)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def same_error(a, b, same):
    return max(float(np.max(np.abs(same[w] - X.same_fft(a[w], b[w])))) for w in range(len(a)))


# ---- 1. every section path: oracle, single call, 'same' span, norms ---------------------------------------------------------------
@pytest.mark.parametrize("na,nb", SHAPES)
def test_rows_against_oracle_single_call_and_scipy(C, na, nb):
    a, b = rows_of(na, nb)
    want_d, want_c, want_s = single(C, a, b)
    assert not want_s.any()
    worst = check_oracle(a, b, want_d, want_c)
    for W in (1, 3):
        d, c, s, norms, same = run_sect(a[:W], b[:W])
        assert same_bits(d, want_d[:W]) and same_bits(c, want_c[:W]) and not s.any(), (W, d, want_d[:W], c, want_c[:W])
        e = same_error(a[:W], b[:W], same)
        print(f"\n{na} x {nb} W {W}: worst lag error of same_out {e:.3e} (twice: {2 * e:.3e}, kXcRivalTol {X.RIVAL_TOL:.1e}); "
              f"worst share of 4 x delay_bounds {worst / A.SAFETY:.3f}", end="")
        assert 2.0 * e <= X.RIVAL_TOL, (na, nb, W, e)
        for w in range(W):                                              # any order of n non-negative terms, and the root
            for k, row in enumerate((a[w], b[w])):
                exact = math.sqrt(math.fsum((row * row).tolist()))
                assert abs(norms[w, k] - exact) <= 2.0 * len(row) * X.U * exact, (w, k, norms[w, k], exact)


# ---- 2. peaks placed by construction ----------------------------------------------------------------------------------------------
def test_peaks_at_the_edges_of_the_span(C):
    na, nb = 3 * S + 5, 2 * S - 1
    wants = (0, 1, 2, na - 3, na - 2, na - 1)
    a = np.stack([X.edge_case(na, nb, w)[0] for w in wants] + [rows_of(na, nb)[0][0]])
    b = np.stack([X.edge_case(na, nb, w)[1] for w in wants] + [rows_of(na, nb)[1][0]])
    d, c, s, _, _ = run_sect(a, b)
    want_d, want_c, want_s = single(C, a, b)
    assert list(s) == [0, 0, 0, 0, 0, 1, 0] and np.array_equal(s, want_s)
    assert np.isnan(d[5]) and np.isnan(c[5])
    ok = s == 0
    assert same_bits(d[ok], want_d[ok]) and same_bits(c[ok], want_c[ok])
    check_oracle(a[ok], b[ok], d[ok], c[ok])
    for w, want in enumerate(wants[:5]):
        assert round(d[w] + na // 2) == want, (w, want, d[w])


def test_peaks_on_the_seams_between_diagonals(C):
    na, nb = 3 * S + 5, 2 * S - 1
    off = (nb - 1) // 2 - (nb - 1)
    wants = [dd * S - off + e for dd in (0, 1) for e in (-1, 0, 1)]     # the lag in samples is j + off = d S - 1, d S, d S + 1
    a = np.stack([X.edge_case(na, nb, w)[0] for w in wants])
    b = np.stack([X.edge_case(na, nb, w)[1] for w in wants])
    d, c, s, _, same = run_sect(a, b)
    want_d, want_c, _ = single(C, a, b)
    assert not s.any() and same_bits(d, want_d) and same_bits(c, want_c)
    check_oracle(a, b, d, c)
    for w, want in enumerate(wants):
        assert round(d[w] + na // 2) == want and int(np.argmax(same[w])) == want
    assert 2.0 * same_error(a, b, same) <= X.RIVAL_TOL


# ---- 3. rivals, ignore_phase, a zero row ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,loud", [(2, 1), (6, 4)])
def test_rivals_are_decided_exactly(C, K, loud):
    """K copies of one template: K - 1 rivals within kXcRivalTol of the top; the louder copy (3e-7) wins, as the oracle says"""
    ra, rb, lags = X.rival_case(K, loud)
    n = len(ra)
    o1 = X.signal_pair("white", n, n, seed=K)
    a, b = np.stack((o1[0], ra)), np.stack((o1[1], rb))
    d, c, s, _, same = run_sect(a, b)
    top, rivals = X.rivals_of(same[1])
    assert len(rivals) == K - 1, (top, rivals)
    o = X.oracle_delay(ra, rb)
    assert o.peak == lags[loud] and round(d[1] + n // 2) == lags[loud]
    want_d, want_c, _ = single(C, a, b)
    assert not s.any() and same_bits(d, want_d) and same_bits(c, want_c)
    check_oracle(a, b, d, c)


def test_ignore_phase_with_the_negative_lobe_on_top(C):
    na, nb = 3 * S + 5, 2 * S - 1
    a, b = rows_of(na, nb)
    a, b = a[:2].copy(), -b[:2]
    d, c, s, _, same = run_sect(a, b, ign=True)
    assert np.all(same[np.arange(2), np.argmax(np.abs(same), axis=1)] < 0)
    want_d, want_c, _ = single(C, a, b, ign=True)
    assert not s.any() and same_bits(d, want_d) and same_bits(c, want_c) and np.all(c < 0)
    check_oracle(a, b, d, c, ign=True)
    d0, c0, _, _, _ = run_sect(a, b, ign=False)
    assert not same_bits(d0, d)


def test_a_row_of_zeros_is_nan_with_status_0(C):
    na, nb = S + 1, S + 1
    a, b = (v.copy() for v in rows_of(na, nb))
    a[1], b[1] = 0.0, 0.0
    d, c, s, norms, _ = run_sect(a, b)
    assert not s.any() and np.isnan(d[1]) and np.isnan(c[1]) and np.all(norms[1] == 0.0)
    want_d, want_c, _ = single(C, a[[0, 2]], b[[0, 2]])
    assert same_bits(d[[0, 2]], want_d) and same_bits(c[[0, 2]], want_c)


# ---- 4. what the results must not depend on ---------------------------------------------------------------------------------------
def test_results_do_not_depend_on_section_scratch_or_run(C):
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    na, nb = 3 * S + 5, 2 * S - 1
    a, b = rows_of(na, nb)
    first = run_sect(a, b, sec=12)
    for sec in (13, 15):
        d, c, s, n, _ = run_sect(a, b, sec=sec)
        assert same_bits(d, first[0]) and same_bits(c, first[1]) and np.array_equal(s, first[2]) and same_bits(n, first[3]), sec
    one = int(L.par_find_delay_sect_scratch_bytes(na, nb, 1, 12))
    assert int(L.par_find_delay_sect_scratch_bytes(na, nb, 3, 12)) == 3 * one
    for nbytes in (one, 2 * one + one // 2):
        got = run_sect(a, b, sec=12, scratch_bytes=nbytes)
        assert all(same_bits(x, y) for x, y in zip(got, first) if x.dtype == np.float64) and np.array_equal(got[2], first[2])
    again = run_sect(a, b, sec=12)
    assert all(same_bits(x, y) for x, y in zip(again, first) if x.dtype == np.float64) and np.array_equal(again[2], first[2])
    with pytest.raises(_lib.ParError, match="less than one row"):
        run_sect(a, b, sec=12, scratch_bytes=one - 1)


def test_the_default_section(C):
    """section_log2 = 0 (2^19 samples): two sections a side, transforms of 2^20 points, W = 2"""
    n = (1 << 19) + 1
    a = np.stack([X.signal_pair("white", n, n, seed=s)[0] for s in (1, 2)])
    b = np.stack([X.signal_pair("white", n, n, seed=s)[1] for s in (1, 2)])
    d, c, s, _, same = run_sect(a, b, sec=0)
    want_d, want_c, _ = single(C, a, b)
    assert not s.any() and same_bits(d, want_d) and same_bits(c, want_c)
    check_oracle(a, b, d, c)
    e = same_error(a, b, same)
    print(f"\n2^19 + 1 samples, section 2^19: worst lag error of same_out {e:.3e} (twice: {2 * e:.3e})", end="")
    assert 2.0 * e <= X.RIVAL_TOL
    import torch
    d2, c2, s2 = C.find_delay_rows_dev(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert same_bits(d2.cpu().numpy(), d) and same_bits(c2.cpu().numpy(), c) and not s2.cpu().numpy().any()     # section None = 19 here


def test_python_wrappers(C):
    na, nb = 3 * S + 5, 2 * S - 1
    a, b = (v.copy() for v in rows_of(na, nb))
    d, c, s, _, _ = run_sect(a, b)
    d1, c1, norms, same = C.find_delay_rows(a, b, section=12, want_norms=True, want_same=True)
    assert same_bits(d1, d) and same_bits(c1, c) and norms.shape == (3, 2) and same.shape == (3, na)
    d2, c2 = C.find_delay_rows(a, b)
    assert same_bits(d2, d) and same_bits(c2, c)
    ea, eb = X.edge_case(na, nb, na - 1)
    with pytest.raises(IndexError, match=r"row 1\)"):
        C.find_delay_rows(np.stack((a[0], ea)), np.stack((b[0], eb)))
