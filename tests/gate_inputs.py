"""Seeded spectra and cutoffs of the renoiser gate tests (test_gate_inputs_cpu.py, test_gate_kernels_gpu.py) and the numpy gate
they are compared with.  No torch, no GPU.

The gate passes a bin when float32(|X|) + 1e-7f >= cutoff.  A kernel whose |X| is an ulp away from np.abs decides differently only
where the cutoff sits ON the magnitude, so the cutoffs here are made from the magnitudes themselves: `cut_on` equals the tie value
m = np.abs(X) + 1e-7f (the tied bin passes; an |X| an ulp too SMALL gates it), `cut_above` is the next float32 above m (the tied bin
is gated; an |X| an ulp too LARGE passes it).  The reference is always np.abs of the numpy in use
(test_renoiser_cpu.py::test_numpy_complex_magnitude_is_the_formula_the_gate_kernels_use guards its formula)."""
import numpy as np

EPS = np.float32(1e-7)
LOW = np.float32(np.power(10, -60.0 / 20))          # renoiser.low_factor(-60)
SENTINEL = np.complex64(-7.5e3 + 2.5e3j)            # pitch padding and guard rows
INF32 = np.float32(np.inf)

_cache = {}


def tie_value(spec):
    """m = float32(np.abs(X)) + 1e-7f: the left side of the gate's comparison"""
    with np.errstate(all="ignore"):
        return (np.abs(np.asarray(spec, dtype=np.complex64)) + EPS).astype(np.float32)


def above(m):
    return np.nextafter(np.asarray(m, dtype=np.float32), INF32)


def passes_np(spec, cut):
    """bool (frames, bins); a NaN on either side compares False: gated"""
    with np.errstate(invalid="ignore"):
        return tie_value(spec) >= np.asarray(cut, dtype=np.float32)[None, :]


def gate_np(spec, cut, low=LOW):
    """spec * where(np.abs(spec) + 1e-7f >= cut, 1, low) in complex64, as numpy multiplies complex64 by float32"""
    fac = np.where(passes_np(spec, cut), np.float32(1.0), np.float32(low)).astype(np.float32)
    with np.errstate(all="ignore"):
        return (np.asarray(spec, dtype=np.complex64) * fac).astype(np.complex64)


def perturbed_magnitude(spec, seed=99, share=0.13):
    """The defect model of the power check: np.abs moved by one float32 ulp, up or down with equal odds, in `share` of the bins
    (a square root that is not correctly rounded; NOTES.md, HPSS, measured 12-14 % for the native instruction)"""
    rng = np.random.default_rng(seed)
    mag = np.abs(np.asarray(spec, dtype=np.complex64)).astype(np.float32)
    hit = rng.random(mag.shape) < share
    up = rng.random(mag.shape) < 0.5
    moved = np.where(up, np.nextafter(mag, INF32), np.nextafter(mag, -INF32)).astype(np.float32)
    return np.where(hit, moved, mag).astype(np.float32)


class Case:
    def __init__(self, name, spec, pitch, cuts):
        self.name, self.spec, self.pitch, self.cuts = name, spec, int(pitch), cuts
        self.spec.setflags(write=False)
        for c in cuts.values():
            c.setflags(write=False)

    @property
    def frames(self):
        return self.spec.shape[0]

    @property
    def bins(self):
        return self.spec.shape[1]

    def pitched(self, pitch=None):
        """(frames, pitch) complex64 with SENTINEL beyond `bins` (pitch 0: the packed rows)"""
        pitch = self.pitch if pitch is None else pitch
        if pitch == 0:
            return np.array(self.spec)
        body = np.full((self.frames, pitch), SENTINEL, dtype=np.complex64)
        body[:, :self.bins] = self.spec
        return body

    def __repr__(self):
        return self.name


# ---- case A: three scaled rows, every bin of row 0 a tie ------------------------------------------------------------------------
A_BINS, A_PITCH = 70001, 70016
A_TINY = slice(30000, 30000 + 4096)                 # |X| of 1e-9 .. 1e-7: the + 1e-7 dominates the tie value


def case_a():
    if "A" not in _cache:
        rng = np.random.default_rng(108)
        scale = 10 ** rng.uniform(-6, 0, A_BINS)
        scale[A_TINY] = 10 ** rng.uniform(-9, -7, 4096)
        row0 = ((rng.standard_normal(A_BINS) + 1j * rng.standard_normal(A_BINS)) * scale).astype(np.complex64)
        spec = np.stack([row0, row0 * np.float32(1.5), row0 * np.float32(0.5)]).astype(np.complex64)
        m = tie_value(row0)
        _cache["A"] = Case("A", spec, A_PITCH, {"on": m, "above": above(m)})
    return _cache["A"]


# ---- case B: more frames than the launch's 4096 grid rows, every bin's median frame a tie ---------------------------------------
B_FRAMES, B_BINS, B_PITCHES = 4101, 515, (0, 520)
GATE_GRID_ROWS = 4096                               # stft.hip par_gate_spectrum_f32: gridDim.y = min(n_frames, 4096)


def median_frame(m):
    """per bin, the frame whose tie value has rank frames // 2 (the median itself for an odd frame count)"""
    return np.argsort(m, axis=0, kind="stable")[m.shape[0] // 2]


def median_cuts(spec):
    m = tie_value(spec)
    cut = m[median_frame(m), np.arange(m.shape[1])]
    return {"on": cut, "above": above(cut)}


def case_b():
    if "B" not in _cache:
        rng = np.random.default_rng(4101)
        shape = (B_FRAMES, B_BINS)
        spec = ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * 10 ** rng.uniform(-6, 0, shape)).astype(np.complex64)
        _cache["B"] = Case("B", spec, 0, median_cuts(spec))
    return _cache["B"]


# ---- case C: special values, each pair of parts under each special cutoff -------------------------------------------------------
C_FRAMES, C_BINS = 4, 300
FLT_MAX = np.finfo(np.float32).max
C_PARTS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-40, 1.1754942e-38, FLT_MAX, -FLT_MAX, 1.0, -3e-8, 1e-7, 2.5e19],
                   dtype=np.float32)                # 1e-45, -1e-40 and 1.1754942e-38 (the largest) are float32 denormals
C_CUTS = np.array([np.nan, np.inf, 0.0, 1e-45], dtype=np.float32)


def case_c():
    """Row 0 holds every ordered pair of C_PARTS as (re, im) (196 bins, then random bins); row r is row 0 rotated by r bins.  The
    cutoffs repeat C_CUTS, and 300 is a multiple of 4: every pair meets all four cutoffs."""
    if "C" not in _cache:
        rng = np.random.default_rng(300)
        re, im = np.meshgrid(C_PARTS, C_PARTS, indexing="ij")
        row0 = (rng.standard_normal(C_BINS) + 1j * rng.standard_normal(C_BINS)).astype(np.complex64)
        pairs = np.empty(re.size, dtype=np.complex64)
        pairs.real, pairs.imag = re.ravel(), im.ravel()
        row0[:pairs.size] = pairs
        spec = np.stack([np.roll(row0, r) for r in range(C_FRAMES)])
        _cache["C"] = Case("C", spec, C_BINS + 4, {"special": np.tile(C_CUTS, C_BINS // 4)})
    return _cache["C"]


def is_denormal(a):
    a = np.abs(np.asarray(a, dtype=np.float32))
    return (a > 0) & (a < np.finfo(np.float32).tiny)


# ---- fused gate: signals ---------------------------------------------------------------------------------------------------------
FUSED_SETTINGS = ((64, 16, 3001), (512, 128, 9001), (2048, 512, 20001), (8192, 2048, 40001),      # (n_fft, hop, n)
                  # 2, 8 and 16 lanes per frame at hop n_fft / 4, one frame more than a workgroup's round holds (128, 32, 16):
                  # (n + n_fft / 2) // hop + 1 frames
                  (32, 8, 1008), (128, 32, 960), (256, 64, 896))


def fused_signal(n, seed=0):
    """float32 noise under a tone: every bin of every frame carries signal, no bin is near the + 1e-7"""
    if ("sig", n, seed) not in _cache:
        rng = np.random.default_rng(1000 + seed)
        t = np.arange(n) / 44100.0
        x = (0.1 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)
        x.setflags(write=False)
        _cache["sig", n, seed] = x
    return _cache["sig", n, seed]


def one_bin_output_change(value, k, n_fft, hop, window, low=LOW):
    """Largest |change| of the least-squares ISTFT's output when bin k (0 < k < n_fft / 2) of ONE interior frame goes from
    `value` to `value * low`: the frame's real inverse transform of the missing part (K_istft undoes K_stft's 1 / sqrt(n_fft)),
    windowed, over the window-sum-square of the frames that cover it."""
    w = np.asarray(window, dtype=np.float64)
    d = np.zeros(n_fft // 2 + 1, dtype=np.complex128)
    d[k] = complex(value) * (1.0 - float(low))
    y = np.fft.irfft(d * np.sqrt(n_fft), n_fft) * w
    wss = np.zeros(n_fft)
    for s in range(-(n_fft // hop) * hop, n_fft, hop):
        lo, hi = max(0, s), min(n_fft, s + n_fft)
        if hi > lo:
            wss[lo:hi] += w[lo - s:hi - s] ** 2
    return float(np.max(np.abs(y) / wss))
