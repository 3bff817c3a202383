"""Closed-form material for the harmonic / percussive separation fixtures (tools/gen_golden_hpss.py) and tests: steady tones
(harmonic), decaying noise bursts (percussive) and a stretch of exact digital silence longer than the widest median window, so
that the soft mask's "both medians below the smallest normal float" branch is taken."""
import numpy as np

SR = 44100
SECONDS = 1.6
SILENCE = (0.55, 1.05)          # seconds: exact zeros; 0.5 s = 172 hops of 128 samples, above the 99 frames of the widest kernel
TONES = ((330.0, 0.20, 0.3), (1245.0, 0.11, 1.1), (3520.0, 0.07, 2.3), (9100.0, 0.03, 0.5))     # Hz, amplitude, phase
BURSTS = (0.08, 0.21, 0.37, 0.50, 1.12, 1.30, 1.47)                                             # seconds
BURST_DECAY = 0.012             # seconds (time constant)


def tones_bursts_silence(seed=109, sr=SR, seconds=SECONDS):
    """(n,) float32"""
    rng = np.random.default_rng(seed)
    n = int(sr * seconds)
    t = np.arange(n) / sr
    x = sum(a * np.sin(2 * np.pi * f * t + p) for f, a, p in TONES)
    noise = rng.standard_normal(n)
    for t0 in BURSTS:
        x = x + 0.4 * noise * np.where(t >= t0, np.exp(-(t - t0) / BURST_DECAY), 0.0)
    x = x.astype(np.float32)
    x[int(SILENCE[0] * sr):int(SILENCE[1] * sr)] = 0.0
    return x


# ------------------------------------------------------------------------------------------------------------------------------
# Value classes for par_hpss_f32 at the ABI (tests/test_hpss_kernels_gpu.py; their properties are proved on the CPU in
# tests/test_hpss_inputs_cpu.py).  Small frame-major arrays (n_frames, bins), float32 or complex64; the magnitudes the kernel
# selects from are np.abs of the array.
AXIS_LENGTHS = (1, 2, 3, 4, 5, 12, 13, 63, 64, 65, 67, 127, 128, 129, 130)      # both sides of the 64-wide tile and of the run of 4
SWEEP_FRAMES = 70                                                               # frames while the lengths sweep along bins
SWEEP_BINS = 66                                                                 # bins while they sweep along frames
CORNER_SHAPES = ((1, 1), (1, 130), (130, 1), (2, 2))
CLASS_SHAPES = ((67, 66), (5, 130), (130, 5))                                   # where the value classes other than `uniform` run
KERNEL_PAIRS = ((1, 1), (2, 3), (3, 2), (4, 5), (5, 4), (31, 17), (98, 99), (99, 98))   # (win_harm, win_perc)
POWERS_EXACT = (2.0, np.inf, 1.0, 0.5)
POWERS_GENERAL = (3.0, 1.5, 0.3, 7.0, 40.0)
MARGINS = ((1.0, 1.0), (2.0, 3.0), (1.1, 1.0))
REAL_CLASSES = ("uniform", "ties", "lowbit", "wide", "nan", "signed")
COMPLEX_CLASSES = ("uniform", "ties", "lowbit", "wide", "nan")

NAN_BITS = 0x7FC00000                   # the positive quiet NaN
INF_BITS = 0x7F800000
FLT_MIN_BITS = 0x00800000
FLT_MAX_BITS = 0x7F7FFFFF
ONE_BITS = 0x3F800000
LOWBIT_BASE = 0x3F9E0650                # 1.2345..., its two lowest bits clear


def f32(bit_patterns):
    return np.asarray(bit_patterns, dtype=np.uint32).view(np.float32)


def uniform(shape, seed):
    return np.random.default_rng(seed).random(shape, dtype=np.float32) * np.float32(4)


def ties(shape, seed):
    """0, 1 and 1 + 1 ulp: every window of three or more holds a value twice"""
    return f32(np.random.default_rng(seed).choice(np.array([0, ONE_BITS, ONE_BITS + 1], np.uint32), size=shape))


def lowbit(shape, seed):
    """one value plus 0..3 ulp: only the last two passes of the bisection tell the elements apart"""
    return f32(np.uint32(LOWBIT_BASE) + np.random.default_rng(seed).integers(0, 4, size=shape, dtype=np.uint32))


def wide_bits(shape, seed):
    rng = np.random.default_rng(seed)
    b = rng.integers(0, INF_BITS, size=shape, dtype=np.uint32)                  # every finite non-negative pattern
    kind = rng.random(shape)
    b = np.where(kind < 0.10, rng.integers(1, FLT_MIN_BITS, size=shape, dtype=np.uint32), b)      # subnormals
    for lo, value in ((0.10, 0), (0.13, FLT_MIN_BITS), (0.16, FLT_MIN_BITS - 1), (0.19, FLT_MAX_BITS), (0.22, INF_BITS), (0.24, 1)):
        b = np.where((kind >= lo) & (kind < lo + 0.03 - 0.01 * (value == INF_BITS)), np.uint32(value), b)
    return b.astype(np.uint32)


def wide(shape, seed):
    return f32(wide_bits(shape, seed))


def nan(shape, seed):
    """`uniform` with about a tenth of the cells NaN, and one whole frame and one whole bin of it"""
    rng = np.random.default_rng(seed + 1000)
    a = uniform(shape, seed).view(np.uint32).copy()
    a[rng.random(shape) < 0.10] = NAN_BITS
    a[shape[0] // 2, :] = NAN_BITS
    a[:, shape[1] // 3] = NAN_BITS
    return f32(a)


def signed(shape, seed):
    """`wide` with random sign bits (-0.0 among them): the kernel reads float32 input through fabsf"""
    rng = np.random.default_rng(seed + 2000)
    return f32(wide_bits(shape, seed) | (rng.integers(0, 2, size=shape, dtype=np.uint32) << np.uint32(31)))


SPECIAL_PARTS = ("nan_x", "x_nan", "pinf_x", "ninf_x", "x_pinf", "x_ninf", "inf_nan")


def plant_special_cells(z, seed):
    """about 1 % of the cells each of (NaN, x), (x, NaN), (+-inf, x), (x, +-inf) and (inf, NaN), x the cell's own other part;
    -> the kind planted per cell (-1: none)"""
    rng = np.random.default_rng(seed + 3000)
    pick = rng.random(z.shape)
    kind = np.full(z.shape, -1)
    nanv, inf = np.float32(np.nan), np.float32(np.inf)
    for i, name in enumerate(SPECIAL_PARTS):
        at = (pick >= 0.012 * i) & (pick < 0.012 * (i + 1))
        kind[at] = i
        re, im = {"nan_x": (nanv, None), "x_nan": (None, nanv), "pinf_x": (inf, None), "ninf_x": (-inf, None), "x_pinf": (None, inf),
                  "x_ninf": (None, -inf), "inf_nan": (inf, nanv)}[name]
        if re is not None:
            z.real[at] = re
        if im is not None:
            z.imag[at] = im
    return kind


def to_complex(mag, seed, special=False):
    """magnitude times a unit phasor: half the cells get one of 1, i, -1, -i (the magnitude survives exactly, so ties and low-bit
    neighbours stay what they are), half a random angle"""
    rng = np.random.default_rng(seed + 4000)
    mag = np.asarray(mag, np.float32)
    theta = rng.uniform(0, 2 * np.pi, mag.shape)
    c, s = np.cos(theta).astype(np.float32), np.sin(theta).astype(np.float32)
    axis = rng.integers(0, 8, mag.shape)
    c = np.where(axis < 4, np.float32([1, 0, -1, 0])[axis % 4], c)
    s = np.where(axis < 4, np.float32([0, 1, 0, -1])[axis % 4], s)
    z = np.empty(mag.shape, np.complex64)
    with np.errstate(all="ignore"):
        z.real, z.imag = mag * c, mag * s
    if special:
        plant_special_cells(z, seed)
    return z


def make(cls, shape, seed, is_complex=False):
    """the array of a class; complex: its complex form, with the special cells planted in `wide` and `nan`"""
    real = {"uniform": uniform, "ties": ties, "lowbit": lowbit, "wide": wide, "nan": nan, "signed": signed}[cls](shape, seed)
    if not is_complex:
        return real
    assert cls != "signed"
    z = to_complex(real, seed, special=cls in ("wide", "nan"))
    if cls == "nan":                                            # the whole frame and the whole bin stay NaN under the planted cells
        z[shape[0] // 2, :] = z[:, shape[1] // 3] = np.complex64(complex(np.nan, np.nan))
    return z


def magnitudes(a):
    with np.errstate(all="ignore"):
        return np.abs(a).astype(np.float32)


# ---- the mask pair table: (harm, perc) pairs reached through 3-wide and 1-wide medians
def _next(bit_pattern, ulps=1):
    return int(bit_pattern) + ulps


X_BITS = 0x3F400000                     # 0.75
LISTED_PAIRS_BITS = (
    (0, 0), (0x00012345, 0x00000777), (FLT_MIN_BITS, 0), (FLT_MIN_BITS - 1, 0), (FLT_MIN_BITS, FLT_MIN_BITS - 1),
    (X_BITS, X_BITS), (X_BITS, _next(X_BITS)),
    (FLT_MAX_BITS, FLT_MAX_BITS - 0x00800000),                  # FLT_MAX, FLT_MAX / 2: times margin 3 the reference is inf, times 2 a tie
    (INF_BITS, ONE_BITS), (ONE_BITS, INF_BITS), (INF_BITS, INF_BITS),
    (NAN_BITS, 0), (0, NAN_BITS), (NAN_BITS, ONE_BITS), (ONE_BITS, NAN_BITS), (NAN_BITS, NAN_BITS), (NAN_BITS, INF_BITS),
    (ONE_BITS, int(np.float32(1e-30).view(np.uint32))), (ONE_BITS, int(np.float32(2.0 ** -20).view(np.uint32))))
N_PAIRS = 70                            # one column per pair: past a 64-wide tile
PAIR_LINES = 68                         # u, u, v, u, u, v, ..., u, u: past a tile too, and the last line is a u


def mask_pairs(seed=1109):
    """(N_PAIRS, 2) float32: the listed (harm, perc) pairs, then log-uniform random ones (values 2^-20 .. 2^20, ratios up to 2^12)"""
    rng = np.random.default_rng(seed)
    listed = f32(np.array(LISTED_PAIRS_BITS, dtype=np.uint32))
    n = N_PAIRS - len(listed)
    u = np.exp2(rng.uniform(-20, 20, n))
    v = u * np.exp2(rng.uniform(-12, 12, n))
    swap = rng.random(n) < 0.5
    rest = np.stack([np.where(swap, v, u), np.where(swap, u, v)], axis=1).astype(np.float32)
    return np.concatenate([listed, rest])


def pair_table(pairs, transposed=False):
    """frame-major float32 array whose medians are the pairs.  Plain: (PAIR_LINES frames, N_PAIRS bins), frames u, u, v, u, u, v, ...
    of column c's pair (u, v); with win_harm = 3, win_perc = 1 a v frame has harm = u, perc = v and a u frame harm = perc = u.
    Transposed: (N_PAIRS frames, PAIR_LINES bins) with win_harm = 1, win_perc = 3: a v cell has harm = v, perc = u."""
    pairs = np.asarray(pairs, np.float32)
    is_v = np.arange(PAIR_LINES) % 3 == 2
    a = np.where(is_v[:, None], pairs[None, :, 1], pairs[None, :, 0]).astype(np.float32)
    return np.ascontiguousarray(a.T) if transposed else a


def pair_table_expected(pairs, transposed=False):
    """(harm, perc) the pair table's medians must be, by the rule in pair_table's docstring"""
    pairs = np.asarray(pairs, np.float32)
    is_v = np.arange(PAIR_LINES) % 3 == 2
    u = np.broadcast_to(pairs[None, :, 0], (PAIR_LINES, len(pairs)))
    own = np.where(is_v[:, None], pairs[None, :, 1], pairs[None, :, 0]).astype(np.float32)
    harm, perc = u.copy(), own
    if transposed:
        return np.ascontiguousarray(own.T), np.ascontiguousarray(harm.T)
    return harm, perc
