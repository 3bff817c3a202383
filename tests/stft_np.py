"""Float64 statements of K_stft / K_istft (csrc/stft.hip) at the C ABI, the restated size dispatch, the yardstick the bounds are
multiples of, the two comparison functions, the inputs and the case tables of tests/test_stft_kernels_gpu.py.  numpy and scipy
only (the guarded device buffers take the torch module from their caller); tests/test_stft_inputs_cpu.py checks all of it without
a GPU, including that the comparison functions reject six kinds of wrong result at the bounds the GPU tests use.

Layout: spectra are FRAME-MAJOR here, (frames, bins), as the ABI writes them; the goldens and oracle_np hold (bins, frames).

What is compared with what.  The reference multiplies window and signal in float32 and transforms the float32 frames; so does the
kernel.  `frames_f32` forms exactly those float32 frames, `stft64` transforms them in float64: what is left between the kernel and
`stft64` is the transform's own rounding, which `yardstick(M)` measures for the reference's backend (pocketfft in float32).

ISTFT comparisons are made in overlap-add units, y * env (`ola_units`): the kernel's rounding lives in the overlap-added frames,
and y is that sum divided by the window-sumsquare envelope, which at the first and last samples of a file (one covering frame) and,
for hop >= n_fft, at every frame edge falls to w[0]^2 = 3.6e-9 for Blackman-Harris.  The division multiplies ANY float32
transform's error by 1 / w there (the reference's pocketfft is 1e-3 of the peak away from float64 at those samples); weighting with
the float64 envelope takes the conditioning out and leaves the kernel's error, which is what R x yardstick bounds.  Under a boxcar
the envelope is a frame count >= 1 and the weighting changes nothing: the boxcar cases pin the envelope paths at full weight."""
import collections
import ctypes
import functools

import numpy as np
import scipy.fft
import scipy.signal

TINY32 = float(np.finfo(np.float32).tiny)
CAP = 2.5e-6                      # no bound may exceed a quarter of the 1e-5 stage contract
MAG_ULP = 2.0 ** -22              # mode 1 on top of the bound, of the value: v_sqrt_f32's 1 ulp and the fused multiply-add
FLOOR_DB = -100.0


# ------------------------------------------------------------------------------------------------ statements
def n_frames_of(n, n_fft, hop):
    return (n + 2 * (n_fft // 2) - n_fft) // hop + 1


def reflect_idx(q, n):
    """np.pad(mode="reflect") index of position q relative to x[0]: period 2 (n - 1); n = 1 -> 0"""
    q = np.asarray(q, dtype=np.int64)
    if n == 1:
        return np.zeros_like(q)
    P = 2 * (n - 1)
    q = np.mod(q, P)
    return np.where(q < n, q, P - q)


def frames_f32(x, n_fft, hop, zeropad, win32):
    """(frames, M) float32: window * reflect-padded slice, the product rounded to float32, zero-extended at the END to M"""
    x = np.asarray(x, dtype=np.float32)
    win32 = np.asarray(win32, dtype=np.float32)
    nf = n_frames_of(len(x), n_fft, hop)
    q = np.arange(nf, dtype=np.int64)[:, None] * hop - n_fft // 2 + np.arange(n_fft, dtype=np.int64)[None, :]
    out = np.zeros((nf, n_fft * zeropad), dtype=np.float32)
    out[:, :n_fft] = win32[None, :] * x[reflect_idx(q, len(x))]
    return out


def stft64(x, n_fft, hop, zeropad, win32):
    return np.fft.rfft(frames_f32(x, n_fft, hop, zeropad, win32).astype(np.float64), axis=1) / np.sqrt(float(n_fft))


def mag64(S):
    return np.abs(S) + 1e-7


IstftOut = collections.namedtuple("IstftOut", "y env ola_len")


def istft64(S, n_fft, hop, win32, y_len, skip):
    """-> (y[y_len] float64, env[y_len] float64 (0 beyond the overlap-add length), ola_len).  irfft drops the imaginary parts of
    bins 0 and H, as numpy's does; the division happens only where the envelope exceeds float32 tiny."""
    S = np.asarray(S).astype(np.complex128)
    nf = S.shape[0]
    assert S.shape[1] == n_fft // 2 + 1
    w = np.asarray(win32, dtype=np.float32).astype(np.float64)
    fr = np.fft.irfft(S * np.sqrt(float(n_fft)), n=n_fft, axis=1) * w[None, :]
    ola_len = n_fft + hop * (nf - 1)
    ola, env = np.zeros(ola_len), np.zeros(ola_len)
    for f in range(nf):
        ola[f * hop:f * hop + n_fft] += fr[f]
        env[f * hop:f * hop + n_fft] += w * w
    nz = env > TINY32
    ola[nz] /= env[nz]
    y, e = np.zeros(y_len), np.zeros(y_len)
    k = max(0, min(y_len, ola_len - skip))
    y[:k], e[:k] = ola[skip:skip + k], env[skip:skip + k]
    return IstftOut(y, e, ola_len)


def ola_units(y, env):
    """y * env where the division happened (module docstring)"""
    return np.asarray(y, dtype=np.float64) * np.where(env > TINY32, env, 1.0)


# ------------------------------------------------------------------------------------------------ dispatch, restated
def ilog2(v):
    l = int(v).bit_length() - 1
    assert 1 << l == v, v
    return l


def stft_variant(n_fft, zeropad, mode, stride, big=None):
    """The kernel a forward call runs.  M = 16384 is served by both entry points: `big` says which (None: par_stft_f32 up to
    16384, as fourier.stft_dev calls them)."""
    M = n_fft * zeropad
    if big is None:
        big = M > 16384
    if not big:
        assert 16 <= M <= 16384
        return ("reg", ilog2(M // 2), int(mode), stride == 1)
    assert M > 8192
    L = ilog2(M // 2)
    if L > 20:
        return ("huge", L - 20)
    l1 = 9 if L == 15 else (8 if L == 14 else (L + 1) // 2)
    return ("four", l1, L - l1)


def fft_geom(logh):
    """-> (lanes per frame, threads, frames per workgroup, padded float2 slots per frame)"""
    H = 1 << logh
    T = H // 8
    threads = max(T, 256)
    return T, threads, threads // T, H + H // 8 + 8


def fused_lds_bytes(n_fft, hop):
    logh = ilog2(n_fft // 2)
    _, _, frames, slots = fft_geom(logh)
    s = -(-n_fft // hop)
    tables = n_fft * 4 + (n_fft // 2) * 8 if logh <= 9 else 0
    return frames * slots * 8 + ((frames * s - 1) * hop + n_fft) * 4 + tables


def is_fused(n_fft, hop):
    return hop >= 1 and 16 <= n_fft <= 2048 and fused_lds_bytes(n_fft, hop) <= 64 * 1024


def istft_variant(n_fft, hop):
    if n_fft > 8192:
        L = ilog2(n_fft // 2)
        return ("big", (L + 1) // 2, L - (L + 1) // 2)
    return ("fused" if is_fused(n_fft, hop) else "frames", ilog2(n_fft // 2))


@functools.lru_cache(maxsize=None)
def largest_fused_hop(n_fft):
    return max(h for h in range(1, 8 * n_fft + 8192) if is_fused(n_fft, h))


def istft_frames_per_group(n_fft):
    return fft_geom(ilog2(n_fft // 2))[2]


# ------------------------------------------------------------------------------------------------ yardstick
def _bh_frames(M):
    w = scipy.signal.get_window("blackmanharris", M).astype(np.float32)
    return (w[None, :] * np.random.default_rng(1000 + ilog2(M)).standard_normal((8, M)).astype(np.float32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def yardstick(M):
    """worst of 8 frames: max_k |rfft_float32 - rfft_float64| / max_k |rfft_float64| with scipy.fft (pocketfft, the reference's backend)"""
    f = _bh_frames(M)
    want = np.fft.rfft(f.astype(np.float64), axis=1)
    got = scipy.fft.rfft(f, axis=1)
    assert got.dtype == np.complex64
    return float(np.max(np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)))


@functools.lru_cache(maxsize=None)
def iyardstick(M):
    """the same for the inverse: scipy.fft.irfft of the complex64 spectra against float64, of each frame's peak"""
    S = np.fft.rfft(_bh_frames(M).astype(np.float64), axis=1)
    want = np.fft.irfft(S.astype(np.complex64).astype(np.complex128), n=M, axis=1)
    got = scipy.fft.irfft(S.astype(np.complex64), n=M, axis=1)
    assert got.dtype == np.float32
    return float(np.max(np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)))


# R per entry point: 3 x the worst ratio (kernel error / yardstick) measured on the MI355X over all cases of the entry point,
# rounded up to the next integer (NOTES.md, "STFT / ISTFT at the ABI"): register STFT 2.64 at M = 16, four-step STFT 2.25 at 2^21,
# ISTFT up to 8192 points 3.75 at n_fft = 512 (hop 33: 16 frames summed in float32), big ISTFT 3.58 at 2^20
R_REG, R_FOUR, R_ISTFT, R_IBIG = 8.0, 7.0, 12.0, 11.0
ALL_M = tuple(1 << k for k in range(4, 22))


def bound(R, M, inverse=False):
    b = R * (iyardstick(M) if inverse else yardstick(M))
    assert b <= CAP, (R, M, b)
    return b


# ------------------------------------------------------------------------------------------------ comparisons
def frame_err(got, want, silent=0.0, allow=0.0):
    """per frame: max_k |got - want| / max_k |want|, after `allow` x |want| has been taken off each difference (mode 1: MAG_ULP).
    A frame whose `want` is `silent` everywhere (0, or 1e-7 in mode 1: nothing but zeros went in) must hold float32(silent)
    exactly: its error is 0 or inf."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.ndim == 2, (got.shape, want.shape)
    out = np.empty(want.shape[0])
    for f in range(want.shape[0]):
        if np.all(want[f] == silent):
            out[f] = 0.0 if np.all(got[f] == got.real.dtype.type(silent)) else np.inf
        else:
            d = np.abs(got[f].astype(want.dtype) - want[f])
            out[f] = np.inf if not np.all(np.isfinite(d)) else np.max(np.maximum(d - allow * np.abs(want[f]), 0.0)) / np.max(np.abs(want[f]))
    return out


def block_err(got, want, block, reach=0):
    """max over blocks of max |got - want| / max(block's peak, file's peak - 100 dB).  The peak is taken over the block widened by
    `reach` samples on either side.  reach = 0 is the block's own peak.  The ISTFT tests pass n_fft - 1: the frames that cover a
    block's samples extend that far beyond it, and a frame's rounding scales with the frame's own peak, so a quiet block within a
    frame length of a loud passage carries the loud frames' rounding in ANY float32 implementation (pocketfft in float32 is 1e-5
    to 3e-5 of such a block's own peak away from float64 on the loud / quiet input, 30 times its error elsewhere)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and got.ndim == 1
    if not np.all(np.isfinite(got)):
        return np.inf
    floor = float(np.max(np.abs(want))) * 10.0 ** (FLOOR_DB / 20.0) if len(want) else 0.0
    worst = 0.0
    for s in range(0, len(want), int(block)):
        d = float(np.max(np.abs(got[s:s + block] - want[s:s + block])))
        ref = max(float(np.max(np.abs(want[max(s - reach, 0):s + block + reach]))), floor)
        worst = max(worst, d / ref if ref > 0.0 else (0.0 if d == 0.0 else np.inf))
    return worst


# ------------------------------------------------------------------------------------------------ inputs
def window32(name, n_fft):
    return scipy.signal.get_window(name, n_fft).astype(np.float32)


def noise(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def loud_quiet(n, seed):
    """the second half is the first half's noise 80 dB down"""
    h = n // 2
    x = np.zeros(n, dtype=np.float32)
    x[:h] = noise(h, seed)
    x[h:2 * h] = x[:h] * np.float32(1e-4)
    return x


def signal(kind, n, seed):
    """kind: noise | loudquiet | const | alt | imp<position> (negative positions count from the end)"""
    if kind == "noise":
        return noise(n, seed)
    if kind == "loudquiet":
        return loud_quiet(n, seed)
    if kind == "const":
        return np.ones(n, dtype=np.float32)
    if kind == "alt":
        return (1.0 - 2.0 * (np.arange(n) % 2)).astype(np.float32)
    assert kind.startswith("imp"), kind
    x = np.zeros(n, dtype=np.float32)
    x[int(kind[3:])] = 1.0
    return x


def istft_spectrum(n_fft, hop, n_frames, win32, seed, kind="noise"):
    """(n_frames, bins) complex64: stft64 of a signal with the band [1, n_fft/4) halved, and imaginary parts in bins 0 and H that
    irfft must ignore"""
    n = hop * (n_frames - 1) + 1
    S = stft64(signal(kind, n, seed), n_fft, hop, 1, win32)[:n_frames].copy()
    assert S.shape[0] == n_frames
    S[:, 1:n_fft // 4] *= 0.5
    S[:, 0] += 1j * (0.25 + 0.5 * np.abs(S[:, 0]))
    S[:, -1] -= 1j * (0.125 + 0.5 * np.abs(S[:, -1]))
    return S.astype(np.complex64)


# ------------------------------------------------------------------------------------------------ case tables
# pitch: "packed" (out_pitch = 0), "plus1" (bins + 1), "round32" (bins rounded up to a multiple of 32)
SCase = collections.namedtuple("SCase", "group n_fft zp hop n mode stride pitch win sig seed")
PITCHES = ("packed", "plus1", "round32")


def pitch_of(kind, bins):
    return {"packed": 0, "plus1": bins + 1, "round32": -(-bins // 32) * 32}[kind]


def _both(group, n_fft, zp, hop, n, win="blackmanharris", sig="noise", strides=(1,), pitches=("packed",), seed=None):
    seed = n_fft + zp + hop + n if seed is None else seed
    return [SCase(group, n_fft, zp, hop, n, m, st, p, win, sig, seed) for m in (0, 1) for st in strides for p in pitches]


def stft_reg_cases():
    c = []
    for k in range(4, 15):                                  # the 44 compiled variants, every pitch form
        M = 1 << k
        c += _both("sweep", M, 1, M // 4, 3 * M + 37, strides=(1, 2), pitches=PITCHES)
    for n_fft, zp in ((2, 8), (4, 4), (8, 2), (256, 2), (1024, 8), (1024, 16)):
        c += _both("zeropad", n_fft, zp, max(n_fft // 4, 1), 5 * n_fft + 3, strides=(1, 2))
    for n_fft in (16, 512, 4096):                           # n < n_fft/2 + 1: frames that fold more than once
        for n in (1, 2, 3, n_fft // 2, n_fft // 2 + 1, n_fft - 1):
            c += _both("short", n_fft, 1, n_fft // 4, n)
    for n_fft, hop, counts in ((16, 1, (1, 255, 256, 257, 2048, 2049)), (512, 128, (7, 8, 9, 63, 64, 65)), (4096, 1024, (1, 7, 8, 9))):
        for nf in counts:                                   # n_frames = n // hop + 1; one frame needs n < hop: n = 1 at hop 2
            c += _both("count", n_fft, 1, hop, hop * (nf - 1) + (hop > 1)) if (nf, hop) != (1, 1) else _both("count", n_fft, 1, 2, 1)
    c += _both("hop", 64, 1, 200, 1500, strides=(1, 2)) + _both("hop", 512, 1, 77, 2000) + _both("hop", 16, 1, 3, 100)
    for M in (16, 512, 8192):
        c += _both("loudquiet", M, 1, M // 4, 8 * M, sig="loudquiet")
        n = 4 * M + 5
        for sig in ("imp0", "imp1", "imp%d" % (M // 2), "imp-1", "const", "alt"):
            c += _both("boxcar", M, 1, M // 4, n, win="boxcar", sig=sig)
    return c


def stft_big_cases():
    """one size per four-step split, both modes, both strides, a misaligned signal; the GUI's zero-padded forms of 2^17"""
    c = []
    for k in range(14, 22):
        M = 1 << k
        hop = M // 4 if k <= 17 else M // 2                 # 5 frames up to 2^17, 3 above: frame 2 (frame 1) is interior
        n = 4 * hop + 37 if k <= 17 else 2 * hop + 37
        c += _both("split", M, 1, hop, n, strides=(1, 2), seed=k)
    for zp in (4, 8, 16):
        c += _both("gui", 1 << 17, zp, 1 << 16, (1 << 17) + 37, seed=30 + zp)
    return c


# y_len: "full" (ola_len - skip), "one", "plus100" (100 samples beyond the overlap-add length); skip None = n_fft / 2
ICase = collections.namedtuple("ICase", "group n_fft hop n_frames win skip y_len sig seed")
FUSED_SIZES = tuple(1 << k for k in range(4, 12))


def odd_hop(n_fft):
    return (n_fft // 3) | 1


def _icase(group, n_fft, hop, nf, win="blackmanharris", skip=None, y_len="full", sig="noise"):
    return ICase(group, n_fft, hop, nf, win, skip, y_len, sig, n_fft + hop + nf)


def count_set(n_fft, hop):
    s, F = -(-n_fft // hop), istft_frames_per_group(n_fft)
    return sorted({v for v in (1, 2, s - 1, s, s + 1, F * s - 1, F * s + 1) if v >= 1})


def istft_cases():
    c = []
    for n_fft in FUSED_SIZES:
        F, top = istft_frames_per_group(n_fft), largest_fused_hop(n_fft)
        for hop in (n_fft // 4, odd_hop(n_fft), n_fft, top, top + 1):
            s = -(-n_fft // hop)
            # more than one workgroup; beyond n_fft the boxcar (envelope 1 inside a frame, module docstring) and skip 0
            c.append(_icase("size", n_fft, hop, F * s + 1, "blackmanharris" if hop < n_fft else "boxcar", 0 if hop > n_fft else None))
    c += [_icase("size", 16, 1, 300), _icase("size", 16, 15, 520)]
    for n_fft, hop in ((16, 4), (256, 64), (512, 33), (1024, 256), (2048, 512)):
        for nf in count_set(n_fft, hop):
            c.append(_icase("count", n_fft, hop, nf, "boxcar", 0))
            c.append(_icase("count", n_fft, hop, nf, "blackmanharris", 0))
    for n_fft, hop, nf in ((512, 128, 30), (2048, 512, 9)):
        ola = n_fft + hop * (nf - 1)
        for win in ("blackmanharris", "hann", "boxcar"):
            for skip in (0, n_fft // 2, n_fft // 2 + 3, ola + 5):
                for y_len in ("one", "full", "plus100"):
                    c.append(_icase("geometry", n_fft, hop, nf, win, skip, y_len))
    c += [_icase("zero_env", 64, 64, 70, "hann", 0), _icase("zero_env", 1024, 1024, 6, "hann", 0)]
    for n_fft in FUSED_SIZES:                               # hop > n_fft with the gaps in the output: exactly +0.0 there
        F = istft_frames_per_group(n_fft)
        c.append(_icase("gap", n_fft, n_fft + 3, 2 * F + 1, "blackmanharris", 0, "plus100"))
        c.append(_icase("gap", n_fft, largest_fused_hop(n_fft), F + 2, "hann", n_fft // 2, "full"))
    c += [_icase("gap", 256, 300, 11, "blackmanharris", None), _icase("gap", 2048, 2592, 4, "boxcar", 0), _icase("gap", 2048, 2593, 4, "boxcar", 0)]
    c += [_icase("frames", 4096, 1024, 6), _icase("frames", 8192, 2048, 5), _icase("frames", 8192, 1001, 5, "boxcar", 0, "plus100"),
          _icase("frames", 16, 15, 300, "boxcar", 0), _icase("frames", 16, 30, 40, "boxcar", 0),
          _icase("frames", 2048, 9697, 3, "hann", 0, "plus100"), _icase("frames", 128, 5000, 4)]
    for n_fft in FUSED_SIZES:                               # loud / quiet, block = hop * Frames
        c.append(_icase("loudquiet", n_fft, n_fft // 4, 8 * istft_frames_per_group(n_fft) + 3, sig="loudquiet"))
    c.append(_icase("loudquiet", 4096, 1024, 12, sig="loudquiet"))
    for k in range(14, 22):
        n_fft = 1 << k
        c.append(_icase("big", n_fft, n_fft // 4, 3 if k <= 19 else 2))
    return c


def icase_geometry(c):
    """-> (skip, y_len, ola_len)"""
    ola = c.n_fft + c.hop * (c.n_frames - 1)
    skip = c.n_fft // 2 if c.skip is None else c.skip
    y_len = {"one": 1, "full": max(ola - skip, 1), "plus100": max(ola - skip, 0) + 100}[c.y_len]
    return skip, y_len, ola


@functools.lru_cache(maxsize=None)
def icase_reference(c):
    """-> (spectrum complex64 (frames, bins), IstftOut) -- computed once per case, shared, never written to"""
    w = window32(c.win, c.n_fft)
    S = istft_spectrum(c.n_fft, c.hop, c.n_frames, w, c.seed, c.sig)
    skip, y_len, ola = icase_geometry(c)
    # never shorter than the overlap-add: a one-sample output is judged against the peak of the frames that made it (the test
    # fills the samples it did not ask for with the reference's own)
    out = istft64(S, c.n_fft, c.hop, w, max(y_len, ola - skip), skip)
    for a in (S, out.y, out.env):
        a.setflags(write=False)
    return S, out


@functools.lru_cache(maxsize=None)
def scase_reference(n_fft, zp, hop, n, win, sig, seed):
    """-> (x float32, stft64) shared by the modes, strides and pitches of a case"""
    x = signal(sig, n, seed)
    S = stft64(x, n_fft, hop, zp, window32(win, n_fft))
    x.setflags(write=False)
    S.setflags(write=False)
    return x, S


def envelope_paths(c):
    """the envelope path of every output sample of a fused case: 0 gap / beyond the overlap-add length, 1 phase table, 2 edge loop
    (at least one covering frame missing), 3 general loop with every frame present (n_fft = 2048 without room for the table)"""
    skip, y_len, ola = icase_geometry(c)
    TT = np.arange(y_len, dtype=np.int64) + skip
    logh = ilog2(c.n_fft // 2)
    _, _, F, slots = fft_geom(logh)
    use_tab = logh <= 9 or c.n_fft + c.hop <= 2 * F * slots
    interior = (TT >= c.n_fft - 1) & (TT <= c.hop * (c.n_frames - 1))
    path = np.where(interior, 1 if use_tab else 3, 2)
    path[(TT >= ola) | (TT % c.hop >= c.n_fft)] = 0
    return path


# ------------------------------------------------------------------------------------------------ guarded device buffers
SENTINEL_BITS = np.uint32(0x7FC5A5A5)          # one quiet-NaN bit pattern: an untouched cell is told from every computed NaN
SENTINEL = np.array([SENTINEL_BITS], dtype=np.uint32).view(np.float32)[0]


def is_sentinel(a):
    return np.ascontiguousarray(a).view(np.uint32) == SENTINEL_BITS


class Guarded:
    """`count` float32 cells on the device between `guard` sentinel cells on either side.  An odd `guard` puts the region 4 bytes
    off the 8-byte grid."""

    def __init__(self, torch, count, body=None, guard=64):
        self.count, self.guard = int(count), int(guard)
        whole = np.full(self.count + 2 * self.guard, SENTINEL, dtype=np.float32)
        if body is not None:
            flat = np.ascontiguousarray(body).view(np.float32).reshape(-1)
            whole[self.guard:self.guard + len(flat)] = flat
        self.before = whole
        self.t = torch.from_numpy(whole.copy()).cuda()

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * self.guard)

    def read(self):
        """-> (the region as float32, both guards still hold the sentinel bit for bit)"""
        now = self.t.cpu().numpy()
        g = self.guard
        ok = bool(is_sentinel(now[:g]).all() and is_sentinel(now[g + self.count:]).all())
        return now[g:g + self.count], ok

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy().view(np.uint32), self.before.view(np.uint32))


def interleave(x, stride):
    """x in channel 0 of `stride` interleaved channels, the sentinel NaN in the others"""
    if stride == 1:
        return np.asarray(x, dtype=np.float32)
    out = np.full((len(x), stride), SENTINEL, dtype=np.float32)
    out[:, 0] = x
    return out.reshape(-1)
