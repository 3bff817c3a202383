"""CPU checks of what tests/test_stft_kernels_gpu.py stands on (tests/stft_np.py): the float64 statements against numpy's own
reflection, the goldens and the pinned oracle; the restated dispatch against the library's host arithmetic; that the case tables
reach every compiled variant and every edge they name; that the comparison functions reject wrong results at the bounds the GPU
tests use; and the argument errors of the three entry points that need no GPU."""
import ctypes
import os

import numpy as np
import pytest
import scipy.fft

import inputs
import stft_np as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def relmax(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


# ------------------------------------------------------------------------------------------------ statements
@pytest.mark.parametrize("n_fft", [16, 64, 512])
def test_reflect_statement_equals_numpy_pad(n_fft):
    pad = n_fft // 2
    for n in (2, 3, 5, n_fft // 2, n_fft // 2 + 1):
        x = np.arange(n, dtype=np.float32) + 1
        want = np.pad(x, pad, mode="reflect")                  # numpy folds as often as it takes when n - 1 < pad
        assert np.array_equal(want, x[N.reflect_idx(np.arange(-pad, n + pad), n)]), (n, n_fft)
    x = np.array([3.0], dtype=np.float32)                      # n = 1: every index is 0 (np.pad reflects a single sample onto itself)
    assert np.array_equal(np.pad(x, pad, mode="reflect"), x[N.reflect_idx(np.arange(-pad, 1 + pad), 1)])


def test_stft64_reproduces_goldens_and_oracle():
    from oracle import oracle_np as O
    g = np.load(os.path.join(GOLDEN, "stft.npz"))
    for name in ("kat1", "bh", "small_vec", "odd_len", "zp2", "zp2_big", "n2048", "n64", "n4096", "hop_eq", "hop_odd"):
        n, seed, n_fft, hop, zp = (int(v) for v in g[name + "_cfg"])
        wname = str(g[name + "_win"])
        x = inputs.noise(n, seed)
        S = N.stft64(x, n_fft, hop, zp, N.window32(wname, n_fft))
        want = g[name + "_S"].T
        assert S.shape == want.shape
        # the golden is the reference's float32 transform: the yardstick is how far that lies from float64
        assert np.max(N.frame_err(want, S)) <= 1.5 * N.yardstick(n_fft * zp), (name, np.max(N.frame_err(want, S)), N.yardstick(n_fft * zp))
        assert np.max(N.frame_err(O.stft(x, n_fft, hop, wname, zp).T, S)) <= 1.5 * N.yardstick(n_fft * zp), name
        assert np.max(N.frame_err(np.abs(want.astype(np.complex128)) + 1e-7, N.mag64(S), 1e-7)) <= 1.5 * N.yardstick(n_fft * zp), name


def test_istft64_reproduces_goldens_and_oracle():
    from oracle import oracle_np as O
    g = np.load(os.path.join(GOLDEN, "istft.npz"))
    for name in ("rt512", "rt1024", "rt256"):
        n, seed, n_fft, hop = (int(v) for v in g[name + "_cfg"])
        x = inputs.noise(n, seed)
        w = N.window32("blackmanharris", n_fft)
        S = O.stft(x, n_fft, hop)                              # what the golden's istft was given (float32 transform, complex128 cells)
        tol = N.yardstick(n_fft) + N.iyardstick(n_fft) + 2.0 ** -22       # + the oracle's float64 window against the ABI's float32 one
        y = N.istft64(S.T, n_fft, hop, w, n, n_fft // 2).y
        assert relmax(y, g[name + "_y"]) <= tol, (name, relmax(y, g[name + "_y"]), tol)
        assert relmax(y, O.istft(S, hop, "blackmanharris", n)) <= tol, name
        S2 = S.copy()
        S2[5:40, 3:9] *= 0.25
        assert relmax(N.istft64(S2.T, n_fft, hop, w, n, n_fft // 2).y, g[name + "_ymod"]) <= tol, name
        nl = hop * (S.shape[1] - 1)
        assert relmax(N.istft64(S.T, n_fft, hop, w, nl, n_fft // 2).y, g[name + "_ynolen"]) <= tol, name


def test_boxcar_inputs_have_the_closed_forms_they_claim():
    for M in (16, 512, 8192):
        w, n, H = N.window32("boxcar", M), 4 * M + 5, M // 2
        mag = np.abs(N.stft64(N.signal("imp%d" % (M // 2), n, 0), M, M // 4, 1, w))
        hit = mag.max(axis=1) > 0
        assert hit.any() and not hit.all()                    # frames without the impulse are all zero: they must come out exactly so
        assert np.allclose(mag[hit], 1 / np.sqrt(M), rtol=1e-12)
        mag = np.abs(N.stft64(N.signal("const", n, 0), M, M // 4, 1, w))
        assert np.allclose(mag[:, 0], np.sqrt(M)) and np.max(mag[:, 1:]) < 1e-10
        mag = np.abs(N.stft64(N.signal("alt", n, 0), M, M // 4, 1, w))
        assert np.allclose(mag[:, H], np.sqrt(M)) and np.max(mag[:, :H]) < 1e-10


# ------------------------------------------------------------------------------------------------ coverage
def test_stft_tables_reach_every_compiled_variant():
    reg = {N.stft_variant(c.n_fft, c.zp, c.mode, c.stride, big=False) for c in N.stft_reg_cases()}
    assert reg == {("reg", lh, m, u) for lh in range(3, 14) for m in (0, 1) for u in (False, True)} and len(reg) == 44
    for pitch in N.PITCHES:                                    # every variant at every pitch form (packed rows at T >= 16: streaming stores)
        assert {N.stft_variant(c.n_fft, c.zp, c.mode, c.stride, big=False) for c in N.stft_reg_cases() if c.pitch == pitch} == reg
    big = N.stft_big_cases()
    assert {N.stft_variant(c.n_fft, c.zp, c.mode, c.stride, big=True) for c in big} == {
        ("four", 7, 6), ("four", 8, 6), ("four", 9, 6), ("four", 8, 8), ("four", 9, 8), ("four", 9, 9), ("four", 10, 9), ("four", 10, 10)}
    for split in {N.stft_variant(c.n_fft, c.zp, c.mode, c.stride, big=True) for c in big}:
        of = [c for c in big if N.stft_variant(c.n_fft, c.zp, c.mode, c.stride, big=True) == split]
        assert {(c.mode, c.stride) for c in of} >= {(0, 1), (0, 2), (1, 1), (1, 2)}, split
    for c in big:                                              # few frames, one of them interior
        nf = N.n_frames_of(c.n, c.n_fft, c.hop)
        assert nf <= 5 and any(f * c.hop - c.n_fft // 2 >= 0 and f * c.hop + c.n_fft // 2 <= c.n for f in range(nf)), c
    assert {c.zp for c in big if c.n_fft == 1 << 17 and c.n_fft * c.zp >= 1 << 19} == {4, 8, 16}


def test_istft_table_reaches_every_variant():
    cases = N.istft_cases()
    got = {N.istft_variant(c.n_fft, c.hop) for c in cases}
    fused = {("fused", lh) for lh in range(3, 11)}
    big = {("big", 7, 6), ("big", 7, 7), ("big", 8, 7), ("big", 8, 8), ("big", 9, 8), ("big", 9, 9), ("big", 10, 9), ("big", 10, 10)}
    frames = {v for v in got if v[0] == "frames"}
    assert got == fused | big | frames
    assert frames >= {("frames", 3), ("frames", 10), ("frames", 11), ("frames", 12)}
    assert N.istft_variant(16, 15) == ("frames", 3) and N.istft_variant(2048, 9697) == ("frames", 10)
    for n_fft in N.FUSED_SIZES:                                # each fused size at the five hops, the last one past the limit
        top = N.largest_fused_hop(n_fft)
        hops = {c.hop for c in cases if c.n_fft == n_fft and c.group == "size"}
        assert hops >= {n_fft // 4, N.odd_hop(n_fft), n_fft, top, top + 1}, n_fft
        assert all(N.is_fused(n_fft, h) for h in (n_fft // 4, N.odd_hop(n_fft), n_fft, top)) and not N.is_fused(n_fft, top + 1)
    assert [N.largest_fused_hop(n) for n in N.FUSED_SIZES] == [29, 75, 167, 350, 716, 1444, 2880, 9696]


def test_restated_fused_rule_is_the_librarys():
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    pairs = [(16, 14), (16, 15), (16, 16), (4096, 1024), (8192, 64), (128, 5000)]
    for n_fft in N.FUSED_SIZES:
        top = N.largest_fused_hop(n_fft)
        pairs += [(n_fft, top), (n_fft, top + 1), (n_fft, 1), (n_fft, n_fft // 4)]
    for n_fft, hop in pairs:
        assert (L.par_istft_scratch_floats(7, n_fft, hop) == 0) == N.is_fused(n_fft, hop), (n_fft, hop)
        if not N.is_fused(n_fft, hop):
            assert L.par_istft_scratch_floats(7, n_fft, hop) == 7 * n_fft
    assert N.is_fused(16, 14) and not N.is_fused(16, 15) and N.is_fused(16, 16)


def test_edge_inputs_hit_what_they_claim():
    reg = N.stft_reg_cases()
    # frames that fold twice or more: an index further than n - 1 outside the signal
    twice = [c for c in reg if c.group == "short" and c.n > 1 and c.n_fft // 2 > 2 * (c.n - 1)]
    assert {c.n_fft for c in twice} == {16, 512, 4096}
    assert any(c.n == 1 for c in reg) and any(c.n == c.n_fft // 2 + 1 for c in reg)
    for n_fft, want in ((16, {1, 255, 256, 257, 2048, 2049}), (512, {7, 8, 9, 63, 64, 65}), (4096, {1, 7, 8, 9})):
        per_group = N.fft_geom(N.ilog2(n_fft // 2))[2]
        counts = {N.n_frames_of(c.n, c.n_fft, c.hop) for c in reg if c.group == "count" and c.n_fft == n_fft}
        assert counts == want, (n_fft, counts)
        assert per_group in counts and (per_group == 1 or {per_group - 1, per_group + 1} <= counts), n_fft
        assert {8 * per_group, 8 * per_group + 1} <= counts, n_fft            # the grid is rounded up to 8 workgroups
    assert N.fft_geom(3)[2] == 256 and N.fft_geom(8)[2] == 8 and N.fft_geom(11)[2] == 1
    assert any(c.hop > c.n_fft for c in reg) and any(c.hop % 2 == 1 and c.hop > 1 for c in reg)
    ic = N.istft_cases()
    # interior range [n_fft - 1, hop (n_frames - 1)] empty and non-empty, and a sample exactly on both hand-over coordinates
    empty = [c for c in ic if N.is_fused(c.n_fft, c.hop) and c.hop * (c.n_frames - 1) < c.n_fft - 1]
    full = [c for c in ic if N.is_fused(c.n_fft, c.hop) and c.hop * (c.n_frames - 1) >= c.n_fft - 1]
    assert empty and full
    for c in [c for c in ic if c.group == "count" and c.n_frames >= -(-c.n_fft // c.hop) + 1]:
        skip, y_len, _ = N.icase_geometry(c)
        assert skip == 0 and y_len > c.hop * (c.n_frames - 1) + 1 and y_len > c.n_fft
        p = N.envelope_paths(c)
        lo, hi = c.n_fft - 1, c.hop * (c.n_frames - 1)
        assert p[lo] == p[hi] == (1 if c.n_fft + c.hop <= 4640 or c.n_fft <= 1024 else 3) and p[lo - 1] == 2 and p[hi + 1] == 2, c
    paths = set()
    for c in ic:
        if N.is_fused(c.n_fft, c.hop):
            paths |= set(np.unique(N.envelope_paths(c)).tolist())
    assert paths == {0, 1, 2, 3}
    # an envelope that is exactly 0: hann (w[0] = 0), hop = n_fft, phase 0
    for c in [c for c in ic if c.group == "zero_env"]:
        S, ref = N.icase_reference(c)
        assert N.window32(c.win, c.n_fft)[0] == 0.0 and np.all(ref.env[::c.hop][:c.n_frames] == 0.0) and np.all(ref.y[::c.hop][:c.n_frames] == 0.0)
    # gap cases have gaps in the output, and some lie in a workgroup other than the first
    for c in [c for c in ic if c.group == "gap"]:
        skip, y_len, ola = N.icase_geometry(c)
        TT = np.arange(y_len) + skip
        gap = (TT % c.hop >= c.n_fft) & (TT < ola)
        assert gap.any(), c
    assert any(c.n_frames > N.istft_frames_per_group(c.n_fft) for c in ic if c.group == "gap")


# ------------------------------------------------------------------------------------------------ the checker rejects what it must
M_REJECT = (16, 512, 8192, 1 << 17)


def pocket32(x, M, hop, w):
    return (scipy.fft.rfft(N.frames_f32(x, M, hop, 1, w), axis=1) / np.float32(np.sqrt(M))).astype(np.complex64)


def r_of(M):
    return N.R_REG if M <= 16384 else N.R_FOUR


@pytest.mark.parametrize("M", M_REJECT)
def test_frame_err_rejects_wrong_spectra(M):
    w, hop, H = N.window32("blackmanharris", M), M // 4, M // 2
    n = 3 * M + 37 if M <= 8192 else M + 37
    x = N.noise(n, M)
    want = N.stft64(x, M, hop, 1, w)
    good = pocket32(x, M, hop, w)
    b = N.bound(r_of(M), M)
    assert np.max(N.frame_err(good, want)) < b
    assert np.max(N.frame_err((np.abs(good) + np.float32(1e-7)).astype(np.float32), N.mag64(want), 1e-7, N.MAG_ULP)) < b
    f = want.shape[0] // 2
    bad = good.copy()                                          # one twiddle-sized error in one bin of one frame
    bad[f, H // 3] += np.float32(1e-5 * np.max(np.abs(want[f])))
    e = N.frame_err(bad, want)
    assert e[f] > b and np.all(np.delete(e, f) < b)
    bad = good.copy()                                          # the pair (k, H - k) swapped
    k = 3
    bad[f, [k, H - k]] = bad[f, [H - k, k]]
    assert N.frame_err(bad, want)[f] > b
    late = N.frames_f32(x, M, hop, 1, w)                       # a frame built one sample late
    q = f * hop - M // 2 + 1 + np.arange(M)
    late[f] = w * x[N.reflect_idx(q, n)]
    bad = (scipy.fft.rfft(late, axis=1) / np.float32(np.sqrt(M))).astype(np.complex64)
    assert N.frame_err(bad, want)[f] > b
    x2 = np.stack([x, N.noise(n, M + 1)], axis=1).reshape(-1)  # the stride ignored
    assert np.max(N.frame_err(pocket32(x2[:n], M, hop, w), want)) > b
    lq = N.loud_quiet(8 * M if M <= 8192 else 4 * M, M)       # the quiet half carrying the loud half at -60 dB
    want = N.stft64(lq, M, hop, 1, w)
    good = pocket32(lq, M, hop, w)
    assert np.max(N.frame_err(good, want)) < b
    half = want.shape[0] // 2
    for leak in (1e-3, 1e-7):                                  # 60 dB under the loud half, and 60 dB under the quiet half itself
        bad = good.copy()
        bad[half + 2:2 * half] += np.complex64(leak) * good[2:half]
        e = N.frame_err(bad, want)
        assert np.all(e[half + 2:2 * half - 2] > b), leak
    assert float(np.max(np.abs(bad - want)) / np.max(np.abs(want))) < 1e-5        # ... which the whole-array metric lets through
    zero = N.stft64(N.signal("imp5", n, 0), M, hop, 1, N.window32("boxcar", M))  # silent frames are held to exact zeros
    leak = zero.astype(np.complex64)
    silent = np.flatnonzero(np.all(zero == 0, axis=1))
    assert len(silent)
    leak[silent[0], 1] = 1e-30
    assert np.isinf(N.frame_err(leak, zero)[silent[0]]) and np.max(N.frame_err(zero.astype(np.complex64), zero)) < b


@pytest.mark.parametrize("n_fft", (16, 512, 2048, 1 << 14))
def test_block_err_rejects_wrong_signals(n_fft):
    hop, w = n_fft // 4, N.window32("blackmanharris", n_fft)
    F = N.istft_frames_per_group(n_fft)
    c = N._icase("loudquiet", n_fft, hop, 8 * F + 3, sig="loudquiet")
    S, ref = N.icase_reference(c)
    skip, _, _ = N.icase_geometry(c)
    y_len = len(ref.y)
    b = N.bound(N.R_ISTFT if n_fft <= 8192 else N.R_IBIG, n_fft, inverse=True)
    block = hop * F
    H = n_fft // 2

    def inverse32(dc_shift=False):
        Sz = S.copy()
        Sz[:, 0].imag = 0
        Sz[:, -1].imag = 0
        fr = scipy.fft.irfft(Sz * np.float32(np.sqrt(n_fft)), n=n_fft, axis=1).astype(np.float32)
        if dc_shift:                                           # the packed inverse with Im X[0] = b and Im X[H] = d left in: Z[0] moves by
            bb, dd = S[:, 0].imag * np.sqrt(n_fft), S[:, -1].imag * np.sqrt(n_fft)       # (-(b + d) + i (b - d)) / 2, every packed point by that / H
            fr[:, 0::2] += (-(bb + dd) / (2 * H))[:, None].astype(np.float32)
            fr[:, 1::2] += ((bb - dd) / (2 * H))[:, None].astype(np.float32)
        ola = np.zeros(n_fft + hop * (c.n_frames - 1))
        for f in range(c.n_frames):
            ola[f * hop:f * hop + n_fft] += (fr[f] * w).astype(np.float32)
        return ola[skip:skip + y_len]                          # overlap-add units already (not divided)

    want = N.ola_units(ref.y, ref.env)
    good = inverse32()
    reach = n_fft - 1
    assert N.block_err(good, want, block, reach) < b
    assert N.block_err(inverse32(dc_shift=True), want, block, reach) > b
    half = y_len // 2
    for leak in (1e-3, 1e-7):                                  # the quiet half carrying the loud half, 60 dB under it / under the quiet half
        bad = good.copy()
        bad[half:2 * half] += leak * good[:half]
        assert N.block_err(bad, want, block, reach) > b, leak
    assert float(np.max(np.abs(bad - want)) / np.max(np.abs(want))) < 1e-5         # ... which the whole-array metric lets through
    bad = good.copy()                                          # one frame leaking into its neighbour's block, 1e-5 of the peak
    bad[2 * block + 1] += 1e-5 * np.max(np.abs(want[2 * block:3 * block]))
    assert N.block_err(bad, want, block, reach) > b


def test_bounds_respect_the_cap_at_every_size():
    for M in N.ALL_M:
        assert N.R_REG * N.yardstick(M) <= N.CAP or M > 16384
        assert N.R_FOUR * N.yardstick(M) <= N.CAP or M < 16384
        assert N.R_ISTFT * N.iyardstick(M) <= N.CAP or M > 8192
        assert N.R_IBIG * N.iyardstick(M) <= N.CAP or M <= 8192


# ------------------------------------------------------------------------------------------------ argument errors without a GPU
def test_argument_errors_of_the_three_entry_points():
    from pyaudiorestoration_amd import _lib
    L, p = _lib.lib(), ctypes.c_void_p(8)
    stft = lambda n_fft, zp, mode=0, pitch=0: L.par_stft_f32(0, p, 100, 1, n_fft, 4, zp, p, p, mode, pitch, None)
    assert stft(64, 1, pitch=32) == 1 and "out_pitch" in _lib.last_error()
    assert stft(64, 2, pitch=64) == 1                          # bins = 65 with the zero padding
    assert stft(64, 1, mode=2) == 1 and "mode" in _lib.last_error()
    assert stft(15, 1) == 3 and stft(2, 4) == 3 and stft(8, 1) == 3 and stft(32768, 1) == 3 and stft(16384, 2) == 3
    assert stft(24, 1) == 3 and stft(3, 16) == 3               # odd n_fft never makes a power of two above 1
    big = lambda n_fft, zp, mode=0, scratch=p, nbytes=1 << 40: L.par_stft_big_f32(0, p, 100, 1, n_fft, 4, zp, p, p, mode, scratch, nbytes, None)
    assert big(8192, 1) == 3 and big(4096, 2) == 3 and big(16384, 1, mode=2) == 1 and big(16384, 1, scratch=None) == 1
    need = L.par_stft_big_scratch_bytes(100, 16384, 4, 1)
    assert need > 0 and big(16384, 1, nbytes=need - 1) == 4 and "scratch" in _lib.last_error()
    ist = lambda n_fft, hop, frames=None: L.par_istft_f32(0, p, 5, n_fft, hop, p, frames, p, 10, 0, None)
    assert ist(8, 2) == 3 and ist(1 << 22, 1 << 20, p) == 3 and ist(48, 12) == 3
    for n_fft, hop in ((4096, 1024), (16, 15), (16384, 4096)):
        assert ist(n_fft, hop) == 1 and "scratch" in _lib.last_error(), (n_fft, hop)
