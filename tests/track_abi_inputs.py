"""Named inputs and numpy statements for the three K_track families (csrc/track.hip) that tests/test_track_abi_gpu.py pins at the
C ABI: k_piptrack (par_piptrack_f32), k_corr_resample / k_corr_peak / k_corr_finish (par_track_corr_f64) and k_zc_*
(par_zero_crossings_f64).  numpy only, no GPU; tests/test_track_abi_inputs_cpu.py proves that every case drives the path it is
named for.

Piptrack.  The kernel forms S = |(mag - offset) * scale| in float32, two rounded operations; `piptrack_statement` forms the same
two in numpy float32 and hands the result to oracle.oracle_np.piptrack, which keeps float32 throughout: pitches and magnitudes
are compared bit for bit.  sr = 48000 and fft_size a power of two make every bin frequency an exact double on both sides.  The
padding of pitched rows holds 3e38: an index that leaves its row reads a value that wins the column maximum.  NaN and inf
magnitudes are outside this pin: np.max propagates a NaN, the kernel's running maximum does not.

Correlation.  The ABI takes the resampling matrix M and the window from its caller, so a test can put a correlation peak on any
lag it likes: `wind` is all ones, M a 0/1 placement matrix (row g holds a single 1 in column b(g), or nothing) and the magnitudes
are small integers.  Every R[i][g] and every un-normalised correlation sum is then an exact integer, ties are exact ties, and the
only rounding left is the division by the norms and the parabola.  Each case names the path it is for (`CorrCase.note`,
`CorrCase.special`).  One realistic case goes through wow_detection.correlation_spline_matrix and np.hanning.

Zero crossings.  Signed zeros, subnormals, NaN and infinities, rotated through the seams of the kernels' 256-sample rounds and
1024-sample tiles; the statement is the reference's own line."""
import collections

import numpy as np

from oracle import oracle_np as O

SR = 48000.0
PAD = np.float32(3e38)

# ================================================================================================ piptrack
PipCase = collections.namedtuple("PipCase", "name mag bins frames pitch fft_size sr fmin fmax threshold scale offset random")


def bin_hz(k, fft_size):
    return k * SR / fft_size                                # exact: sr = 375 * 2^7, fft_size a power of two


def pitched(a, pad):
    """[frames][cols] -> [frames][cols + pad], the padding filled with 3e38"""
    out = np.full((a.shape[0], a.shape[1] + pad), PAD, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


def hand_columns(bins):
    """nine frames of hand-built columns on `bins` >= 60 bins (values are exact in float32 and survive scale 1, offset 0)"""
    z = np.zeros((9, bins), dtype=np.float32)
    z[0, 9:13] = (0.25, 1.0, 1.0, 0.25)                     # plateau of two: bin 10 is the peak, bin 11 is not
    z[0, 30:35] = (0.25, 0.75, 0.75, 0.75, 0.5)             # plateau of three: bin 31 alone
    z[1, :4] = (2.0, 1.0, 0.5, 0.25)                        # the maximum on bin 0: never a pitch (no left neighbour to exceed)
    z[1, 20:23] = (0.5, 1.5, 0.75)
    #   frame 2 stays all zero
    z[3, 19:22] = (0.25, 1.0, 0.125)                        # threshold 0.5: 1.0 is the maximum,
    z[3, 29:32] = (0.25, 0.5, 0.125)                        # 0.5 == 0.5 * 1.0 is NOT above the reference value
    z[4, 19:22] = (0.25, 1.0, 0.375)                        # both raw neighbours under the threshold: the local maximum is taken on
    z[4, 25:28] = (0.125, 0.625, 0.25)                      # the thresholded column, the parabola on the raw one
    z[5, bins - 3:] = (0.25, 0.5, 1.0)                      # the last bin is the maximum above its left neighbour (shift 0)
    z[5, 15:18] = (0.5, 0.75, 0.25)
    for k in (5, 8, 40, 45):                                # peaks below, on fmin (8), on fmax (40) and above it
        z[6, k - 1:k + 2] = (0.375, 1.0, 0.625)
    z[7, 6:10] = (0.5, 1.0, 1.0, 0.625)                     # a plateau that starts on fmin's left neighbour: bin 8 is no peak
    z[7, 39:42] = (1.0, 1.0, 0.5)                           # bin 39 is the peak of a plateau that ends on fmax
    z[8] = np.where(np.arange(bins) % 4 == 2, 1.0, 0.5)     # a peak every fourth bin
    return z


def random_columns(seed, frames, bins, quantised, zeros=0.3):
    """seeded magnitudes in [0, 1) with a share of exact zeros; quantised: the SAME numbers rounded to eighths (ties are common)"""
    rng = np.random.default_rng(seed)
    u = rng.random((frames, bins))
    keep = rng.random((frames, bins)) >= zeros
    if quantised:
        u = np.rint(u * 8) / 8
    return (u * keep).astype(np.float32)


def _pip_cases():
    out = []

    def add(name, mag, fft_size, fmin, fmax, threshold=0.1, scale=1.0, offset=0.0, pad=0, random=False):
        frames, bins = mag.shape
        assert bins <= fft_size // 2 + 1
        m = pitched(mag, pad) if pad else mag.copy()
        m.setflags(write=False)
        out.append(PipCase(name, m, bins, frames, bins + pad, fft_size, SR, float(fmin), float(fmax), float(threshold),
                           np.float32(scale), np.float32(offset), random))

    # hand-built columns: limits exactly on bin frequencies with the last bin below Nyquist; the same columns with open limits
    add("hand_on_bins", hand_columns(65), 256, bin_hz(8, 256), bin_hz(40, 256), threshold=0.5, pad=37)
    add("hand_open", hand_columns(65), 128, -100.0, 1e6, threshold=0.5)
    add("hand_below_nyquist_open", hand_columns(65), 1024, -1.0, 30000.0, threshold=0.5)
    # seeded columns, every bin count x frame count x row pitch, quantised and not; (scale, offset): (1, 0), the wrapper's defaults,
    # and in "below_offset" an offset about 5 % of the cells lie under
    table = [  # bins frames pad fft_size fmin fmax scale offset
        (2, 1, 0, 2, -1.0, 1e9, 1.0, 0.0),
        (2, 3, 37, 8, 0.0, 24000.0, None, 1e-7),
        (3, 4, 37, 4, -5.0, 24001.0, 1.0, 0.0),
        (3, 5, 0, 16, 0.0, 1e5, None, 1e-7),
        (63, 5, 0, 128, bin_hz(3, 128), bin_hz(60, 128), 1.0, 0.0),
        (63, 9, 37, 256, -10.0, bin_hz(62, 256), None, 1e-7),
        (64, 9, 37, 256, bin_hz(1, 256), bin_hz(63, 256), None, 1e-7),
        (64, 1, 0, 128, 0.0, 1e9, 3.0, 0.0),
        (65, 3, 0, 128, bin_hz(2, 128), 24000.0, None, 1e-7),
        (65, 4, 37, 512, -1.0, 1e9, 1.0, 0.0),
        (129, 5, 37, 256, bin_hz(5, 256), bin_hz(120, 256), 1.0, 0.0),
        (129, 4, 0, 1024, 0.0, bin_hz(128, 1024), None, 1e-7),
        (257, 4, 0, 1024, bin_hz(7, 1024), 1e9, None, 1e-7),
        (257, 9, 37, 512, -3.0, bin_hz(200, 512), 1.0, 0.0),
    ]
    for i, (bins, frames, pad, fft_size, fmin, fmax, scale, offset) in enumerate(table):
        scale = np.float32(np.sqrt(fft_size)) if scale is None else scale
        for q in (True, False):
            mag = random_columns(100 + i, frames, bins, q)
            if offset:                                      # what get_mag hands over: |stft| / sqrt(n_fft) + 1e-7, in float32
                mag = mag / np.float32(np.sqrt(fft_size)) + np.float32(offset)
            add(f"rand_b{bins}_f{frames}_p{pad}_n{fft_size}_{'q8' if q else 'raw'}", mag, fft_size, fmin, fmax, scale=scale,
                offset=offset, pad=pad, random=True)
    # about 5 % of the cells lie below the offset: S is negative there before the abs.  Threshold 0.01, so that such a cell can be
    # a peak; one is planted in frame 0 (0.03 under the offset between cells 0.01 and 0.005 from it)
    for bins, frames, pad, fft_size, q in ((129, 5, 0, 256, False), (65, 9, 37, 256, True)):
        off = 0.0625 if q else 0.05
        mag = random_columns(200 + bins, frames, bins, q, zeros=0.0)
        if not q:
            mag = np.maximum(mag, np.float32(1e-3))
        mag[0, 50:55] = (off + 0.004, off + 0.01, off - 0.03, off - 0.005, off + 0.002)
        add(f"below_offset_b{bins}_{'q8' if q else 'raw'}", mag, fft_size, 0.0, 1e9, threshold=0.01, scale=3.0, offset=off, pad=pad,
            random=True)
    return out


PIP_CASES = _pip_cases()


def pip_S32(c):
    """|(mag - offset) * scale| in numpy float32, (frames, bins): the two rounded operations of the kernel"""
    return np.abs((c.mag[:, :c.bins] - np.float32(c.offset)) * np.float32(c.scale))


def piptrack_statement(c, S32=None):
    """-> (pitches, mags), float32 (frames, bins), from oracle_np.piptrack on the float32 S"""
    S32 = pip_S32(c) if S32 is None else S32
    assert S32.dtype == np.float32
    p, m = O.piptrack(S32.T, c.sr, c.fft_size, fmin=c.fmin, fmax=c.fmax, threshold=np.float32(c.threshold))
    assert p.dtype == np.float32 and m.dtype == np.float32
    return np.ascontiguousarray(p.T), np.ascontiguousarray(m.T)


# ================================================================================================ correlation
# special: {pair index: ("tie", lowest lag, the other lags) | ("nan",) | ("lag0",) | ("last_lag",)}
CorrCase = collections.namedtuple("CorrCase", "name note mag bins n_frames NL NU nb n count M wind special integer")


def placement(n, nb, col):
    """M[g][col[g]] = 1 (col[g] < 0: the row stays zero)"""
    M = np.zeros((n, nb))
    g = np.arange(n)
    M[g[col >= 0], col[col >= 0]] = 1.0
    return M


def _corr_case(name, note, col, bands, nb, bins=None, NL=2, NU=None, n_frames=None, special=None, junk=7.0):
    """bands: [count][nb] small integers; the bins outside the band hold `junk`, frames behind `count` hold 3e38"""
    bands = np.asarray(bands, dtype=np.float64)
    count = len(bands)
    n = len(col)
    NU = NL + n // 4 if NU is None else NU
    bins = NU + 3 if bins is None else bins
    n_frames = count if n_frames is None else n_frames
    assert n == 4 * (NU - NL) and nb == min(NU, bins) - NL and bands.shape == (count, nb)
    mag = np.full((n_frames, bins), PAD, dtype=np.float32)
    mag[:count] = junk
    mag[:count, NL:NL + nb] = bands
    mag.setflags(write=False)
    return CorrCase(name, note, mag, bins, n_frames, NL, NU, nb, n, count, placement(n, nb, np.asarray(col)), np.ones(n),
                    special or {}, True)


def nearest_layout(n, nb):
    """every grid point takes the nearest band value: a piecewise-constant resampling"""
    return np.rint(np.arange(n) * (nb - 1) / (n - 1)).astype(np.int64)


def bump_bands(seed, count, nb, peaks):
    """positive integers: a seeded floor of 1 .. 3 with a bump (+6, +3 beside it) on bin peaks[i]"""
    rng = np.random.default_rng(seed)
    b = rng.integers(1, 4, (count, nb)).astype(np.float64)
    for i, p in enumerate(peaks):
        for d, v in ((-1, 3), (0, 6), (1, 3)):
            if 0 <= p + d < nb:
                b[i, p + d] += v
    return b


# columns of the placed layouts: three-point bumps A, B, D, and the two grid ends (E1: points 0, 1; E2: points n-2, n-1).  A frame
# whose grid ends are not zero has a single best lag against the all-ones frame behind the last one.
A, B, D, E1, E2 = 0, 3, 6, 9, 10
PLACED_NB = 11


def placed_layout(n, where):
    """where: {first column of a three-point bump: [first grid point, ...], E1 / E2: True}"""
    col = np.full(n, -1, dtype=np.int64)
    for c, starts in where.items():
        if c in (E1, E2):
            pts = (0, 1) if c == E1 else (n - 2, n - 1)
            assert np.all(col[list(pts)] < 0)
            col[list(pts)] = c
            continue
        for s in starts:
            assert np.all(col[s:s + 3] < 0) and s + 3 <= n, (c, s)
            col[s:s + 3] = (c, c + 1, c + 2)
    return col


def frame(nb, **groups):
    v = np.zeros(nb)
    for name, vals in groups.items():
        c = {"A": A, "B": B, "D": D, "E1": E1, "E2": E2}[name]
        vals = np.atleast_1d(vals)
        v[c:c + len(vals)] = vals
    return v


def _corr_cases():
    out = []
    # ---- sizes: nb = 3 is the smallest band the ABI accepts; n below one wave, just over one wave, just over 256 threads (threads
    # own one or two lags), threads owning two and three lags; count 1 (the only pair is with the all-ones frame) and 2
    for nb, count, peaks in ((3, 1, (1,)), (3, 2, (0, 2)), (5, 3, (1, 3, 2)), (17, 4, (5, 9, 8, 12)), (65, 3, (20, 40, 33)),
                             (129, 3, (90, 30, 64))):
        out.append(_corr_case(f"sizes_nb{nb}_n{4 * nb}_c{count}", "band and grid sizes", nearest_layout(4 * nb, nb),
                              bump_bands(nb, count, nb, peaks), nb))
    # ---- a band clipped at the last bin: nb = bins - NL values, the grid keeps 4 (NU - NL) points, M is [n][nb]
    out.append(_corr_case("clipped_band", "NL > 0, NU > bins", nearest_layout(52, 8), bump_bands(8, 3, 8, (2, 5, 4)), 8, bins=20, NL=12,
                          NU=25))
    # ---- count < n_frames: the frames behind `count` hold 3e38 and are not read
    out.append(_corr_case("count_below_n_frames", "count < n_frames", nearest_layout(68, 17), bump_bands(17, 3, 17, (4, 11, 9)), 17,
                          n_frames=5))
    nb = 17
    # ---- the peak on lag 0: frame 0's bump on grid points 0..2, frame 1's on n/2..n/2+2, frame 0's grid end not zero so that
    # f[n-1], which parabolic() wraps to, is neither 0 nor f[1]
    n = 68
    col = placed_layout(n, {A: [0], B: [n // 2], E2: True})
    out.append(_corr_case("peak_on_lag_0", "parabolic()'s f[-1] wrap", col,
                          [frame(nb, A=(1, 3, 2), E2=1), frame(nb, B=(2, 3, 1)), frame(nb, A=(1, 1, 1), B=(1, 3, 2), E2=2)], nb,
                          special={0: ("lag0",)}))
    # ---- the peak on lag n-1: PAR_ERR_INDEX from the ABI, IndexError from the statement
    col = placed_layout(n, {A: [n // 2 + 1], B: [2], E1: True, E2: True})
    out.append(_corr_case("peak_on_last_lag", "status bit 2", col,
                          [frame(nb, A=(1, 3, 2)), frame(nb, B=(2, 3, 1)), frame(nb, B=(1, 3, 2), E1=1, E2=2)], nb,
                          special={0: ("last_lag",)}))

    def tie_case(name, note, n, nb, pa, pbs, lags, extra=None, closing=None, winner=None):
        where = {A: [pa], B: list(pbs), E1: True, E2: True}
        second = frame(nb, B=(2, 3, 1))
        last = frame(nb, B=(1, 3, 2), E1=1, E2=2)
        if extra is not None:
            where[D] = [extra]
            second += frame(nb, D=(4, 6, 2))
            last += frame(nb, D=(2, 6, 4))
        sp = ("tie", min(lags), tuple(sorted(lags)[1:])) if winner is None else ("tie_below_max", winner, tuple(sorted(lags)))
        out.append(_corr_case(name, note, placed_layout(n, where), [frame(nb, A=(1, 3, 2)), second, last], nb, special={0: sp}))
    # ---- exact ties (frame 1 holds the same bump twice): lag = n/2 + pa - pb
    tie_case("tie_lags_5_200", "lanes in different waves", 260, 65, 100, (30, 225), (5, 200))
    tie_case("tie_lags_3_35", "lanes of one wave", 260, 65, 10, (105, 137), (3, 35))
    tie_case("tie_lags_10_266", "the same thread (lags j and j + 256)", 516, 129, 250, (242, 498), (10, 266))
    # ---- a tie in the last wave (lags 200 and 230) under a higher value on lag 100: the maximum wins, not the first seen
    tie_case("tie_under_the_maximum", "the maximum wins", 260, 65, 150, (50, 80), (200, 230), extra=180, winner=100)
    # ---- a silent band at frame 3 of 6: its norm is 0, every lag of pairs 2 and 3 is NaN, np.argmax returns the first NaN
    n = 68
    col = placed_layout(n, {A: [20], B: [40], E1: True, E2: True})
    fa, fb = frame(nb, A=(1, 3, 2)), frame(nb, B=(2, 3, 1))
    out.append(_corr_case("silent_frame_3_of_6", "first NaN wins", col, [fa, fb, fa, frame(nb), fa, frame(nb, B=(2, 3, 1), E1=1, E2=2)],
                          nb, special={2: ("nan",), 3: ("nan",)}, junk=0.0))
    return out


def _realistic_cases():
    """the wrapper's own M and window on seeded float32 magnitudes: a bump that moves by a fraction of a bin per frame"""
    from pyaudiorestoration_amd.wow_detection import correlation_spline_matrix
    out = []
    for nb, NL in ((7, 5), (33, 12)):
        NU, bins, count = NL + nb, NL + nb + 6, 5
        n = 4 * nb
        log_f = np.log2(np.arange(NL, NU) * SR / 1024)
        rng = np.random.default_rng(nb)
        k = np.arange(bins)[None, :]
        centre = NL + nb / 2 + np.cumsum(rng.uniform(-0.4, 0.4, count))[:, None]
        mag = (np.exp(-0.5 * ((k - centre) / (0.15 * nb + 0.8)) ** 2) + 0.05 * rng.random((count, bins))).astype(np.float32)
        mag.setflags(write=False)
        out.append(CorrCase(f"realistic_nb{nb}", "spline matrix, Hann window", mag, bins, count, NL, NU, nb, n, count,
                            correlation_spline_matrix(log_f, n), np.hanning(n), {}, False))
    return out


CORR_CASES = _corr_cases()
CORR_REALISTIC = _realistic_cases()


def corr_rows(c):
    """R: [(count + 1)][n] float64 = (M @ band) * wind per frame, then one row equal to wind"""
    band = c.mag[:c.count, c.NL:c.NL + c.nb].astype(np.float64)
    return np.concatenate(((c.M @ band.T).T * c.wind[None, :], c.wind[None, :]), axis=0)


def corr_same(c, R=None):
    """same[i][j]: np.correlate's 'same' lags of rows i and i + 1 (exact for the integer cases) over the product of their norms"""
    R = corr_rows(c) if R is None else R
    out = np.empty((c.count, c.n))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(c.count):
            a, b = R[i], R[i + 1]
            s = np.correlate(a, b, "same")
            out[i] = s / (np.sqrt(np.sum(a * a)) * np.sqrt(np.sum(b * b)))
    return out


def first_argmax(v):
    return int(np.argmax(v))                                # first occurrence; the first NaN when there is one


def corr_statement(c):
    """-> dict(R, same, peaks, changes, cum).  Raises IndexError where the reference's parabolic() does (a peak on lag n-1)."""
    R = corr_rows(c)
    same = corr_same(c, R)
    peaks = np.array([first_argmax(s) for s in same])
    changes = np.empty(c.count)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(c.count):
            refined, _ = O.parabolic(same[i], int(peaks[i]))        # wraps to f[-1] at lag 0, IndexError at lag n-1
            changes[i] = c.n // 2 - refined
    return {"R": R, "same": same, "peaks": peaks, "changes": changes, "cum": np.cumsum(changes)}


def corr_oracle_refined(c, i, R=None):
    """the refined peak of pair i by oracle_np.xcorr / parabolic: ties the statement to the oracle"""
    R = corr_rows(c) if R is None else R
    r = O.xcorr(R[i], R[i + 1], "same")
    return O.parabolic(r, int(np.argmax(r)))[0]


# ================================================================================================ zero crossings
ZC_SEQUENCE = np.array([+0.0, -0.0, 5e-324, -5e-324, np.nan, 1.0, np.nan, -1.0, np.inf, -np.inf, 0.0])


def _zc_vectors():
    """the sequence repeated over 2100 samples (two tile seams, eight round seams) in each of its 11 rotations, so that every
    adjacent pair of it lands on every seam; and short prefixes"""
    out = {}
    reps = 2100 // len(ZC_SEQUENCE) + 2
    for r in range(len(ZC_SEQUENCE)):
        out[f"rot{r}_n2100"] = np.tile(np.roll(ZC_SEQUENCE, r), reps)[:2100].copy()
    for n in (2, 11, 256, 257, 1024, 1025):
        out[f"rot0_n{n}"] = np.tile(ZC_SEQUENCE, reps)[:n].copy()
    return out


ZC_VECTORS = _zc_vectors()


def zc_statement(x):
    return np.where(np.bitwise_xor(x[1:] > 0, x[:-1] > 0))[0]
