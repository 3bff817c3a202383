"""Seeded inputs of the tracker tests (test_tracker_inputs_cpu.py, test_trackers_gpu.py) and the two replays both files
assert on: the band sequence the oracle's Center of Gravity walks, and how far every band edge the oracle rounds lies
from a rounding cliff.

The GPU tests compare K_track with oracle.oracle_np.TRACKERS on the SAME magnitudes, so the only way the two may part is
a band edge int(round(f * fft_size / sr)) whose argument sits within a libm ulp (about 1e-13 bins) of a half-integer.  The
CPU file proves the inputs keep 1e-6 bins away from every such cliff: a band that differs on the GPU is a kernel error.
"""
import numpy as np
import scipy.signal

from oracle import oracle_np as O

WINDOW = "blackmanharris"
CLIFF_MARGIN = 1e-6                     # bins; one ulp of a libm difference moves a rounded argument by about 1e-13
TRACKERS = ("Peak", "Peak Track", "Center of Gravity", "Correlation")


# ------------------------------------------------------------------------------------------ signals
def glide(n, fa, fb):
    return fa * (fb / fa) ** (np.arange(n) / (n - 1))


def vib(n, sr, f0, depth, rate):
    return f0 * (1 + depth * np.sin(2 * np.pi * rate * np.arange(n) / sr))


def tone(n, sr, f, dc=0.0, noise=1e-3, seed=0):
    """0.5 sin(phase of the instantaneous frequency f) + dc + noise; f a scalar or one value per sample."""
    f = np.broadcast_to(np.asarray(f, dtype=np.float64), (n,))
    return (0.5 * np.sin(2 * np.pi * np.cumsum(f) / sr) + dc
            + noise * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


class Case:
    def __init__(self, name, sr, n_fft, hop, x, trail, tol, zeropad=1):
        self.name, self.sr, self.n_fft, self.hop, self.x, self.tol, self.zeropad = name, sr, n_fft, hop, x, tol, zeropad
        self._trail = [(float(t), float(f)) for t, f in trail]

    @property
    def trail(self):                    # trackers sort the trail in place: every caller gets a list of its own
        return list(self._trail)

    @property
    def fft_size(self):                 # what the trackers are told: the zero-extended transform
        return self.n_fft * self.zeropad

    @property
    def bins(self):
        return self.fft_size // 2 + 1

    def __repr__(self):
        return self.name


def _named(name, sr, n_fft, hop, dur, law, trail, tol, **kw):
    n = int(dur * sr)
    return Case(name, sr, n_fft, hop, tone(n, sr, law(n, sr), **kw), trail, tol)


_BUILDERS = {
    "glide3": lambda: _named("glide3", 48000, 2048, 512, 1.0, lambda n, sr: glide(n, 3500.0, 5500.0),
                             [(0, 3500), (1.0, 5500)], 3.0),
    "wide4": lambda: _named("wide4", 48000, 2048, 256, 0.5, lambda n, sr: glide(n, 6000.0, 6400.0),
                            [(0, 6000), (0.5, 6400)], 4.0),
    "vib64": lambda: _named("vib64", 48000, 2048, 256, 0.75, lambda n, sr: vib(n, sr, 4310.0, 0.05, 5.0),
                            [(0.05, 4310), (0.7, 4310)], 3.0),
    "narrow1": lambda: _named("narrow1", 48000, 1024, 128, 0.5, lambda n, sr: glide(n, 3000.0, 5000.0),
                              [(0, 3000), (0.5, 5000)], 1.0),
    "down": lambda: _named("down", 44100, 512, 64, 0.4, lambda n, sr: glide(n, 9000.0, 3000.0),
                           [(0, 9000), (0.4, 3000)], 1.0),
    "bin0": lambda: _named("bin0", 48000, 256, 64, 0.25, lambda n, sr: 300.0, [(0.02, 300), (0.2, 300)], 0.2, dc=0.6),
    # two more trail shapes on one short glide: a start of exactly 0 with an end past the file (frame_1 clipped to the
    # spectrogram), and a span of one frame
    "clipped_end": lambda: _named("clipped_end", 48000, 1024, 256, 0.5, lambda n, sr: glide(n, 4000.0, 4100.0),
                                  [(0.0, 4000), (5.0, 4100)], 0.5),
    "one_frame": lambda: _named("one_frame", 48000, 1024, 256, 0.5, lambda n, sr: glide(n, 4000.0, 4100.0),
                                [(0.3, 4050), (0.3 + 1.5 * 256 / 48000, 4050)], 0.5),
}
NAMED = ("glide3", "wide4", "vib64", "narrow1", "down", "bin0")
TRAIL_SHAPES = ("clipped_end", "one_frame")
_cache = {}


def case(name):
    """A named case; built once, its signal shared (read-only) by every test."""
    if name not in _cache:
        c = _BUILDERS[name]()
        c.x.setflags(write=False)
        _cache[name] = c
    return _cache[name]


# Seeds of the sweep.  A seed whose bands come within CLIFF_MARGIN of a rounding cliff is REPLACED here by another seed
# (test_tracker_inputs_cpu.py::test_no_band_edge_on_a_rounding_cliff says which); it is never given a looser bound.
SWEEP_SEEDS = tuple(range(1000, 1032))


def sweep_case(seed):
    """A shortened form of tools/fuzz_trackers.py's generator: random rate, transform, hop (one that does not divide
    n_fft among them), a glide with a little vibrato in noise, a 2-5 point shuffled trail that follows the pilot."""
    if ("sweep", seed) in _cache:
        return _cache["sweep", seed]
    rng = np.random.default_rng(seed)
    sr = int(rng.choice([44100, 96000, 192000]))
    n_fft = int(rng.choice([256, 512, 1024, 2048]))
    hop = int(rng.choice([n_fft // 8, n_fft // 4, n_fft // 2, n_fft // 4 + 3]))
    dur = float(rng.uniform(0.2, 0.5))
    n = int(sr * dur)
    f0 = float(rng.uniform(800, min(12000, sr / 4)))
    inst = glide(n, f0, f0 * float(rng.uniform(0.8, 1.25))) * vib(n, sr, 1.0, float(rng.uniform(0.001, 0.01)),
                                                                  float(rng.uniform(2, 12)))
    x = tone(n, sr, inst, noise=10 ** float(rng.uniform(-4, -1)), seed=seed)
    ts = rng.uniform(0.02 * dur, 0.98 * dur, int(rng.integers(2, 6)))          # unsorted: the trackers sort
    if rng.random() < 0.25:
        ts[np.argmin(ts)] = 0.0
    if rng.random() < 0.25:
        ts[np.argmax(ts)] = 1.5 * dur
    trail = [(float(t), float(inst[min(n - 1, int(t * sr))] * rng.uniform(0.995, 1.005))) for t in ts]
    tol = float(rng.choice([0.2, 0.5, 1.0, 3.0]))
    c = Case(f"sweep{seed}", sr, n_fft, hop, x, trail, tol)
    c.x.setflags(write=False)
    _cache["sweep", seed] = c
    return c


def oracle_mag(c):
    """The oracle's own spectrogram rounded through float32: the CPU stand-in for the device's."""
    return O.get_mag(c.x, c.n_fft, c.hop, WINDOW, c.zeropad).astype(np.float32).astype(np.float64)


# (n_fft, hop, zeropad, seconds) of the refined Peak / Peak Track runs: fewer samples than the kernel's 256 threads, a
# zero-extended transform, a hop that does not divide n_fft, several turns of the twiddle recurrence.  The trail spans the
# file, so the first and the last traced frame reflect at the signal's ends.
REFINED = ((256, 64, 1, 0.1), (64, 16, 4, 0.05), (1024, 100, 2, 0.2), (4096, 1024, 1, 0.5))


def refined_case(n_fft, hop, zp, dur):
    key = ("refined", n_fft, hop, zp, dur)
    if key not in _cache:
        sr = 48000
        n = int(dur * sr)
        c = Case(f"refined_{n_fft}_{hop}_{zp}", sr, n_fft, hop, tone(n, sr, glide(n, 4000.0, 4400.0)),
                 [(0, 4000), (dur, 4400)], 1.0, zeropad=zp)
        c.x.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def float64_mag(c):
    """The exact spectrum of the reference's float32 frames: its window and frame matrix (reflect padding, product rounded
    to float32), transformed in float64 -- what k_track_peak_refined evaluates, by numpy's rfft."""
    win = scipy.signal.get_window(WINDOW, c.n_fft).astype(np.float32)
    xp = np.pad(c.x, c.n_fft // 2, mode="reflect")
    idx = np.arange((len(xp) - c.n_fft) // c.hop + 1)[:, None] * c.hop + np.arange(c.n_fft)[None, :]
    frames = (win[None, :] * xp[idx]).astype(np.float32).astype(np.float64)
    return (np.abs(np.fft.rfft(frames, n=c.fft_size, axis=1)) / np.sqrt(c.n_fft) + 1e-7).T


# ------------------------------------------------------------------------------------------ replays
def cog_bands(spec, c):
    """The (NL, NU) Center of Gravity reduces per frame and its result BEFORE NaN patching, replayed with the oracle's
    geometry (oracle_np.track_cog's loop; the CPU file checks the replay against track_cog itself)."""
    g = O._TrackGeometry(spec, c.trail, c.fft_size, c.hop, c.sr, c.tol)
    ff = O.fft_freqs(c.fft_size, c.sr)
    bands, raw = [], np.empty(len(g.freqs))
    g.limits(*g.band(g.freqs[0]))
    with np.errstate(all="ignore"):
        for i in range(len(raw)):
            bands.append((g.NL, g.NU))
            w = np.hanning(g.NU - g.NL) * spec[g.NL:g.NU, g.frame_0 + i]
            raw[i] = 2 ** (np.sum(w * np.log2(ff[g.NL:g.NU])) / np.sum(w))
            g.limits(*g.band(raw[i]))
    return bands, raw


def band_stats(bands):
    """What the walk of k_track_cog depends on: widths, changes of band (cached terms and prefetch go stale), and
    crossings of the 64-bin width between its two loops."""
    L = np.array([nu - nl for nl, nu in bands])
    wide = L > 64
    return {"frames": len(bands), "min_L": int(L.min()), "max_L": int(L.max()), "wide": int(wide.sum()),
            "changes": sum(a != b for a, b in zip(bands, bands[1:])), "crossings": int((wide[1:] != wide[:-1]).sum())}


def peak_argmax_bins(spec, c):
    """The bin Peak's argmax lands on, per frame."""
    g = O._TrackGeometry(spec, c.trail, c.fft_size, c.hop, c.sr, c.tol)
    out = []
    for i in range(len(g.freqs)):
        g.limits(*g.band(g.freqs[i]))
        out.append(g.NL + int(np.argmax(spec[g.NL:g.NU, g.frame_0 + i])))
    return out


def _edge_args(g, freq, tol=None):
    fL, fU = g.band(freq, tol)
    return [max(1.0, fL) * g.fft_size / g.sr, min(g.sr / 2, fU) * g.fft_size / g.sr]


def cliff_margin(spec, c):
    """Smallest distance, in bins, of any argument the oracle rounds to a band edge from a half-integer: Peak's
    per-frame trail frequency, Peak Track's two tolerances on freqs[0], Center of Gravity's per-frame result."""
    g = O._TrackGeometry(spec, c.trail, c.fft_size, c.hop, c.sr, c.tol)
    if len(g.freqs) == 0:
        return np.inf
    args = []
    for f in g.freqs:
        args += _edge_args(g, f)
    args += _edge_args(g, g.freqs[0]) + _edge_args(g, g.freqs[0], g.tol / 2)
    with np.errstate(all="ignore"):
        for f in cog_bands(spec, c)[1]:
            args += _edge_args(g, f)                      # a NaN result leaves the clamps: 1 Hz and Nyquist
    a = np.array(args) - 0.5
    return float(np.min(np.abs(a - np.rint(a))))


# precondition rows of the named cases, asserted on the oracle's spectrogram (CPU) and again on the device's (GPU):
# lower bounds set loosely below what the oracle's band sequence showed, since the two spectrograms differ in the last
# float32 bit
def assert_paths(name, spec, c):
    bands, raw = cog_bands(spec, c)
    s = band_stats(bands)
    if name == "glide3":
        assert s["wide"] >= 30 and s["crossings"] >= 1 and s["changes"] >= 60, s
    elif name == "wide4":
        assert s["min_L"] > 64 and s["changes"] >= 20, s
    elif name == "vib64":
        assert s["crossings"] >= 6, s
    elif name in ("narrow1", "down"):
        assert s["changes"] >= 50 and s["max_L"] <= 64, s
    elif name == "bin0":
        L = [nu - nl for nl, nu in bands]
        assert bands[0] == (0, 4), bands[0]
        assert np.isnan(raw).sum() >= 1, raw
        assert c.bins - 2 in L, s
        assert 0 in peak_argmax_bins(spec, c)
    elif name == "clipped_end":
        assert s["frames"] == spec.shape[1], s              # frame_1 clipped to the spectrogram
    elif name == "one_frame":
        assert s["frames"] == 1, s
    return s, raw
