"""Seeded inputs and float64 numpy oracles of the K_heal tests (test_heal_inputs_cpu.py, test_heal_kernels_gpu.py): the six
entry points of csrc/heal.hip, each against a plain restatement of the reference operation it stands for.  No torch, no GPU.

The GPU tests compare cell by cell, so the inputs must keep away from the two places where a 1e-13 dB difference between two
float64 evaluations may legitimately change the result: an unclipped gain of 0 (written or not) and of 255 (clipped or not).
The CPU file proves every case keeps 1e-6 dB away from both; a seed that does not is REPLACED here, its cells are never
filtered out.
"""
import numpy as np
from scipy.interpolate import RegularGridInterpolator

GAIN_MAX = 255.0                # np.clip(g, previous, 255), dropout_healer_gui.py:157
CLIP_MARGIN = 1e-6              # dB
K_GAIN_BINS = 256               # heal.hip kGainBins: bins per workgroup of k_inpaint_gain, threads per workgroup
K_COPY_SPAN = 2048              # heal.hip kCopySpan: copied samples per workgroup of k_copy_segments


# ------------------------------------------------------------------------------------------ inpaint mask
def marker_valid(m, n_frames, bins):
    """What the kernels let through (heal.hip:45, :88-90; pipeline._check_geometry is the host mirror): the box and its
    surrounding frames inside the spectrogram, a non-empty band inside [0, bins]."""
    fb, fa, fs, bl, bu = m
    return fs >= 1 and fa - fb >= 1 and fb - fs >= 0 and fa + fs <= n_frames and bl >= 0 and bu <= bins and bu > bl


def _db(spec_fm):
    """to_dB(to_mag(S)) of the reference on its (bins, frames) layout, float64 / complex128"""
    S = np.asarray(spec_fm).astype(np.complex128).T
    with np.errstate(all="ignore"):
        return 20 * np.log10(np.abs(S) + .0000001)


def gain_mask_np(spec_fm, markers, preset=None):
    """The reference's serial marker loop (oracle_np.heal_dropouts :552-567 without the time / frequency conversion) on a
    frame-major complex64 spectrogram -> (frames, bins) float64 mask.  RegularGridInterpolator on the 2-frame grid, one value
    column per bin (the reference's second grid axis runs over the band's own bins and only ever evaluates ON them), then
    np.clip(g, previous, 255).  `preset`: what the mask holds before the first marker (zeros in the reference)."""
    n_frames, bins = spec_fm.shape
    db = _db(spec_fm)
    gain_whole = np.zeros(db.shape) if preset is None else np.asarray(preset, dtype=np.float64).T.copy()
    for m in markers:
        if not marker_valid(m, n_frames, bins):
            continue
        frame_b, frame_a, fs, bin_l, bin_u = (int(v) for v in m)
        with np.errstate(all="ignore"):
            before = np.mean(db[bin_l:bin_u, frame_b - fs:frame_b], axis=1)
            after = np.mean(db[bin_l:bin_u, frame_a:frame_a + fs], axis=1)
            fp_frames = np.linspace(frame_b, frame_a, num=frame_a - frame_b)
            interp = RegularGridInterpolator(((frame_b, frame_a),), np.stack((before, after)))
            fp_db = np.swapaxes(interp(fp_frames[:, None]), 0, 1)
            g = fp_db - db[bin_l:bin_u, frame_b:frame_a]
            np.clip(g, gain_whole[bin_l:bin_u, frame_b:frame_a], GAIN_MAX, out=g)
        gain_whole[bin_l:bin_u, frame_b:frame_a] = g
    return np.ascontiguousarray(gain_whole.T)


def marker_gains_np(spec_fm, markers):
    """[(marker, unclipped gain (nf, nb))] of the valid markers, the closed form's way: tt = i / (nf - 1)"""
    n_frames, bins = spec_fm.shape
    db = _db(spec_fm).T
    out = []
    for m in markers:
        if not marker_valid(m, n_frames, bins):
            continue
        fb, fa, fs, bl, bu = (int(v) for v in m)
        nf = fa - fb
        with np.errstate(all="ignore"):
            before = np.mean(db[fb - fs:fb, bl:bu], axis=0)
            after = np.mean(db[fa:fa + fs, bl:bu], axis=0)
            tt = (np.arange(nf) / (nf - 1) if nf > 1 else np.zeros(1))[:, None]
            out.append((tuple(int(v) for v in m), before[None] * (1.0 - tt) + after[None] * tt - db[fb:fa, bl:bu]))
    return out


def unclipped_max_np(spec_fm, markers):
    """max_k g_k per cell, -inf outside every box"""
    u = np.full(spec_fm.shape, -np.inf)
    for (fb, fa, fs, bl, bu), g in marker_gains_np(spec_fm, markers):
        u[fb:fa, bl:bu] = np.maximum(u[fb:fa, bl:bu], g)
    return u


def gain_mask_closed_np(spec_fm, markers, preset=None):
    """min(255, max(0, max_k g_k)) -- the identity k_inpaint_gain's atomic max relies on (a preset takes the place of 0)"""
    base = np.zeros(spec_fm.shape) if preset is None else np.asarray(preset, dtype=np.float64)
    return np.maximum(base, np.minimum(GAIN_MAX, unclipped_max_np(spec_fm, markers)))


def box_cells(shape, markers):
    """bool (frames, bins): inside the box of at least one valid marker"""
    inside = np.zeros(shape, dtype=bool)
    for m in markers:
        if marker_valid(m, *shape):
            inside[m[0]:m[1], m[3]:m[4]] = True
    return inside


def apply_np(spec, mask):
    with np.errstate(invalid="ignore"):                     # the poison cases: NaN and Inf pass through
        return np.asarray(spec).astype(np.complex128) * 10 ** (np.asarray(mask, dtype=np.float64) / 20)


def kernel_geometry(m):
    """The thread geometry k_inpaint_gain and k_apply_gain_boxes derive from a marker, computed the way they compute it:
    per chunk of 256 bins (nbc, P = 256 // nbc); the apply kernel's single P."""
    fb, fa, fs, bl, bu = (int(v) for v in m)
    nb = bu - bl
    chunks = []
    b0 = bl
    while b0 < bu:
        nbc = min(bu - b0, K_GAIN_BINS)
        chunks.append((nbc, K_GAIN_BINS // nbc))
        b0 += K_GAIN_BINS
    return {"nb": nb, "fs": fs, "nf": fa - fb, "chunks": len(chunks), "nbc": tuple(c[0] for c in chunks),
            "P": tuple(c[1] for c in chunks), "apply_P": K_GAIN_BINS // nb if nb < K_GAIN_BINS else 1,
            "apply_loops": nb >= K_GAIN_BINS}


class Case:
    """A synthetic frame-major spectrogram with its markers.  `expect`: the facts of kernel_geometry(markers[0]) (and of the
    case as a whole) it exists for, asserted by the CPU file."""

    def __init__(self, name, spec, markers, expect=None, preset=None):
        self.name, self.spec, self.expect, self.preset = name, spec, expect or {}, preset
        self.markers = [tuple(int(v) for v in m) for m in markers]
        self.spec.setflags(write=False)
        if preset is not None:
            self.preset.setflags(write=False)

    @property
    def frames(self):
        return self.spec.shape[0]

    @property
    def bins(self):
        return self.spec.shape[1]

    def __repr__(self):
        return self.name


def noise_spec(seed, frames, bins):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((frames, bins)) + 1j * rng.standard_normal((frames, bins))).astype(np.complex64)


def dropout_spec(seed, frames, bins, markers, scale=1e-3):
    """complex64 noise, the frames of every valid box multiplied by `scale` (a number, or one per marker)"""
    spec = noise_spec(seed, frames, bins)
    scales = np.broadcast_to(np.asarray(scale, dtype=np.float32), (len(markers),))
    done = np.zeros(frames, dtype=bool)
    for m, s in zip(markers, scales):
        if marker_valid(m, frames, bins):
            rows = np.arange(m[0], m[1])
            rows = rows[~done[rows]]
            spec[rows] *= s
            done[rows] = True
    return spec


def _one(name, seed, frames, bins, marker, **expect):
    return Case(name, dropout_spec(seed, frames, bins, [marker]), [marker], expect)


def _width(nb, seed, bins=300, bin_l=3, **expect):
    # fs = 5 surrounding frames, a box of 7: frames 8 .. 15 of 24
    return _one(f"nb{nb}", seed, 24, bins, (8, 15, 5, bin_l, bin_l + nb), nb=nb, **expect)


def _clip_case(name, box):
    """surroundings at |z| >= 1e6 around exact zeros (`clip255`): -140 dB in the box under >= 120 dB around it, an unclipped gain
    >= 260.  `clip255_tiny` has |z| = 1e-9 .. 2e-9 in the box instead (-139.9 dB), so that the apply kernel's 10^(255/20) meets
    a number it can be measured on."""
    rng = np.random.default_rng(77)
    frames, bins, m = 24, 300, (9, 14, 4, 20, 120)
    mag = 1e6 * (1 + rng.random((frames, bins)))
    ph = rng.uniform(0, 2 * np.pi, (frames, bins))
    spec = (mag * np.exp(1j * ph)).astype(np.complex64)
    spec[m[0]:m[1]] *= np.float32(box)
    return Case(name, spec, [m], {"all_clipped": True, "box": box})


def _preset_case():
    frames, bins, m = 24, 300, (8, 15, 5, 10, 110)
    pre = np.zeros((frames, bins), dtype=np.float32)
    pre[8:11, 10:60] = 200.0            # above the new gain (about 60 dB): stays
    pre[11:15, 40:110] = 1.5            # below: replaced
    pre[2, 7] = 3.25                    # outside every box: stays
    return Case("preset", dropout_spec(31, frames, bins, [m]), [m], {"preset": True}, preset=pre)


def _invalid_case():
    frames, bins = 40, 300
    ms = [(10, 16, 4, 5, 90),           # valid
          (3, 8, 4, 5, 90),             # frame_b - fs = -1
          (30, 37, 4, 5, 90),           # frame_a + fs = n_frames + 1
          (20, 26, 5, 100, 260),        # valid
          (10, 16, 4, -1, 90),          # bin_l = -1
          (10, 16, 4, 200, 301),        # bin_u = bins + 1
          (12, 12, 4, 5, 90),           # nf = 0
          (10, 16, 0, 5, 90),           # fs = 0
          (10, 16, 4, 90, 90),          # bin_u == bin_l
          (10, 16, 4, 95, 90),          # bin_u < bin_l
          (28, 36, 4, 0, 300)]          # valid: flush against the last frame, the whole row
    valid = [ms[0], ms[3], ms[10]]
    return Case("invalid", dropout_spec(41, frames, bins, valid), ms, {"valid": 3, "invalid": 8})


def _many_case():
    """64 random boxes in one launch, attenuations between 1e-3 and 1 so that gains of both signs occur"""
    rng = np.random.default_rng(64)
    frames, bins = 96, 513
    ms = [_random_marker(rng, frames, bins) for _ in range(64)]
    return Case("many64", dropout_spec(65, frames, bins, ms, 10 ** rng.uniform(-3, 0, 64)), ms, {"markers": 64})


def _random_marker(rng, frames, bins):
    fs = int(rng.integers(1, 9))
    nf = int(rng.integers(1, min(20, frames - 2 * fs) + 1))
    fb = int(rng.integers(fs, frames - fs - nf + 1))
    nb = int(min(bins, rng.choice([1, 2, 7, 40, 64, 99, 128, 200, 256, 300, 700])))
    bl = int(rng.integers(0, bins - nb + 1))
    return (fb, fb + nf, fs, bl, bl + nb)


_BUILDERS = {
    # ---- band width: P = 256 // nb frame lanes per bin, chunks of 256 bins
    "nb1": lambda: _width(1, 1, P=(256,)),
    "nb3": lambda: _width(3, 2, P=(85,)),
    "nb85": lambda: _width(85, 3, P=(3,)),
    "nb86": lambda: _width(86, 4, P=(2,)),
    "nb128": lambda: _width(128, 5, P=(2,)),
    "nb129": lambda: _width(129, 6, P=(1,)),
    "nb255": lambda: _width(255, 7, P=(1,), apply_loops=False),
    "nb256": lambda: _width(256, 8, P=(1,), chunks=1, apply_loops=True),
    "nb257": lambda: _width(257, 9, chunks=2, nbc=(256, 1), P=(1, 256), apply_loops=True),
    "nb925": lambda: _width(925, 10, bins=1025, bin_l=50, chunks=4, nbc=(256, 256, 256, 157), P=(1, 1, 1, 1), apply_loops=True),
    "row257": lambda: _width(257, 11, bins=257, bin_l=0, chunks=2, nbc=(256, 1)),
    "row1025": lambda: _width(1025, 12, bins=1025, bin_l=0, chunks=5, nbc=(256, 256, 256, 256, 1)),
    # ---- surrounding frames against P = 6 (40 bins)
    "fs1": lambda: _one("fs1", 13, 24, 100, (8, 15, 1, 30, 70), P=(6,), fs=1),
    "fs_lt_P": lambda: _one("fs_lt_P", 14, 24, 100, (8, 15, 4, 30, 70), P=(6,), fs=4, fs_lt_P=True),
    "fs_not_mult": lambda: _one("fs_not_mult", 15, 32, 100, (10, 17, 8, 30, 70), P=(6,), fs=8, fs_mod_P=2),
    "fs_mult": lambda: _one("fs_mult", 16, 40, 100, (14, 21, 12, 30, 70), P=(6,), fs=12, fs_mod_P=0),
    # ---- box length against P = 6
    "nf1": lambda: _one("nf1", 17, 24, 100, (10, 11, 5, 30, 70), P=(6,), nf=1),
    "nf2": lambda: _one("nf2", 18, 24, 100, (10, 12, 5, 30, 70), P=(6,), nf=2),
    "nf_lt_P": lambda: _one("nf_lt_P", 19, 24, 100, (10, 14, 5, 30, 70), P=(6,), nf=4, nf_lt_P=True),
    "nf_not_mult": lambda: _one("nf_not_mult", 20, 40, 100, (10, 25, 5, 30, 70), P=(6,), nf=15, nf_mod_P=3),
    # ---- placement
    "flush_start": lambda: _one("flush_start", 21, 24, 100, (5, 12, 5, 30, 70), start=0),
    "flush_end": lambda: _one("flush_end", 22, 24, 100, (12, 19, 5, 30, 70), end=24),
    # ---- marker sets
    "overlap": lambda: (lambda ms: Case("overlap", dropout_spec(23, 48, 300, ms, [.3, .05, .5, 1e-3, .1]), ms, {"overlap": True}))(
        [(10, 20, 5, 20, 120), (12, 18, 3, 40, 80), (15, 30, 6, 100, 290), (16, 17, 2, 0, 300), (8, 22, 8, 60, 61)]),
    "twice": lambda: (lambda m: Case("twice", dropout_spec(24, 24, 100, [m]), [m, m], {"twice": True}))((8, 15, 5, 30, 70)),
    "many64": _many_case,
    # ---- clipping
    "clip255": lambda: _clip_case("clip255", 0.0),
    "clip255_tiny": lambda: _clip_case("clip255_tiny", 1e-15),
    "louder": lambda: (lambda m: Case("louder", dropout_spec(25, 24, 300, [m], 1e3), [m], {"none_written": True}))((8, 15, 5, 10, 110)),
    # ---- pre-set mask, invalid markers
    "preset": _preset_case,
    "invalid": _invalid_case,
}
NAMED = tuple(_BUILDERS)
_cache = {}


def case(name):
    """A named case; built once, shared read-only"""
    if name not in _cache:
        _cache[name] = _BUILDERS[name]()
    return _cache[name]


# Seeds of the sweep.  A seed with a cell inside CLIP_MARGIN of 0 or 255 is REPLACED here
# (test_heal_inputs_cpu.py::test_margins_at_the_clips names it); the margin stays.
SWEEP_SEEDS = tuple(range(2000, 2024))


def sweep_case(seed):
    """1-6 random valid boxes (they may overlap) on noise, attenuated by 1e-3 .. 3 so that gains of both signs occur"""
    if ("sweep", seed) not in _cache:
        rng = np.random.default_rng(seed)
        frames = int(rng.integers(20, 97))
        bins = int(rng.choice([65, 257, 300, 513, 1025]))
        ms = [_random_marker(rng, frames, bins) for _ in range(int(rng.integers(1, 7)))]
        scale = 10 ** rng.uniform(-3, 0.5, len(ms))
        _cache["sweep", seed] = Case(f"sweep{seed}", dropout_spec(seed + 1, frames, bins, ms, scale), ms)
    return _cache["sweep", seed]


def all_cases():
    return [case(n) for n in NAMED] + [sweep_case(s) for s in SWEEP_SEEDS]


def max_fs(c):
    return max(abs(m[2]) for m in c.markers)


# poison values: (case, bin, expected mask of that bin's box cells by the reference)
def poison_case(kind):
    """`nan` / `nan_neg`: one NaN (either sign bit) in a frame before the box of bin 57, which an overlapping second marker
    covers too; `inf`: one Inf there.  -> (Case, bin, marker order variants)"""
    if ("poison", kind) not in _cache:
        ms = [(10, 16, 4, 40, 80), (12, 20, 3, 50, 70)]
        spec = dropout_spec(51, 32, 100, ms).copy()
        if kind == "inf":
            spec[8, 57] = np.complex64(complex(np.inf, 0.0))
        else:
            re = np.array([0x7fc00000 if kind == "nan" else 0xffc00000], dtype=np.uint32).view(np.float32)[0]
            spec[8, 57] = np.complex64(complex(re, 1.0))
        _cache["poison", kind] = Case(f"poison_{kind}", spec, ms)
    return _cache["poison", kind], 57


# ------------------------------------------------------------------------------------------ band mean
def band_mean_db_np(mag, bl, bu, fb, fa):
    with np.errstate(divide="ignore"):
        return np.mean((20 * np.log10(np.asarray(mag).astype(np.float64)))[fb:fa, bl:bu], axis=1)


def band_mag(seed, frames, bins):
    """float32 magnitudes between 1e-7 and 1e7 (-140 .. 140 dB)"""
    rng = np.random.default_rng(seed)
    return (10 ** rng.uniform(-7, 7, (frames, bins))).astype(np.float32)


# ------------------------------------------------------------------------------------------ curve scale / accumulate
# (n, frames): a single sample, a single knot, two of each, every sample on a knot (97, 97), n - 1 a multiple of
# frames - 1 (13, 4), (7, 3), several workgroups
CURVE_SHAPES = ((1, 1), (1, 5), (2, 2), (5, 64), (97, 97), (13, 4), (7, 3), (100001, 7))
CHANNELS = ((1, 1), (2, 2), (3, 3), (1, 2), (2, 5), (3, 4))          # (n_ch, sig_stride)


def curve_case(n, frames, n_ch, stride):
    """-> sig (n, stride) float32, fac (n_ch, frames) float64 (factor - 1 of the heuristic: 0 .. 30, some knots exactly 0)"""
    rng = np.random.default_rng(n * 1000 + frames * 10 + n_ch + stride)
    sig = rng.standard_normal((n, stride)).astype(np.float32)
    fac = 10 ** rng.uniform(-2, 1.5, (n_ch, frames)) - 0.01
    fac[rng.random((n_ch, frames)) < 0.2] = 0.0
    return sig, fac


def curve_scale_np(sig, fac):
    n, frames = sig.shape[0], fac.shape[1]
    return np.stack([sig[:, c].astype(np.float64) * np.interp(np.linspace(0, 1, n), np.linspace(0, 1, frames), fac[c])
                     for c in range(fac.shape[0])])


def curve_scale_bound(sig, fac):
    """8 * 2**-53 * |sig_i| * (M_i + (frames - 1) * D_i), M_i the largest |fac| and D_i the largest |delta fac| over the
    intervals [k, k + 1] / (frames - 1) that touch x_i = i / (n - 1) -- decided in integers: k (n - 1) <= i (frames - 1)
    <= (k + 1) (n - 1)."""
    n, frames = sig.shape[0], fac.shape[1]
    out = np.empty((fac.shape[0], n))
    i = np.arange(n, dtype=np.int64)
    for c in range(fac.shape[0]):
        a = np.abs(fac[c])
        if frames == 1 or n == 1:
            M, D = np.full(n, a[0]), np.zeros(n)
        else:
            t = i * (frames - 1)
            lo = np.clip(-(-t // (n - 1)) - 1, 0, frames - 2)          # ceil - 1
            hi = np.clip(t // (n - 1), 0, frames - 2)
            d = np.abs(np.diff(fac[c]))
            m = np.maximum(a[:-1], a[1:])
            M, D = np.maximum(m[lo], m[hi]), np.maximum(d[lo], d[hi])
        out[c] = 8 * 2.0 ** -53 * np.abs(sig[:, c].astype(np.float64)) * (M + (frames - 1) * D)
    return out


def accumulate_case(n, n_ch, stride):
    """-> sig (n, stride) float32, y (n_ch, n) float64; the first samples are exact float32 ties: 1 + 2^-24 (to even: down),
    (1 + 2^-23) + 2^-24 (to even: up), and their negatives"""
    rng = np.random.default_rng(n * 100 + n_ch * 10 + stride)
    sig = rng.standard_normal((n, stride)).astype(np.float32)
    y = rng.standard_normal((n_ch, n)) * 10 ** rng.uniform(-8, 1, (n_ch, n))
    ties = [(1.0, 2.0 ** -24), (1.0 + 2.0 ** -23, 2.0 ** -24), (-1.0, -2.0 ** -24), (-1.0 - 2.0 ** -23, -2.0 ** -24)]
    for k, (s, d) in enumerate(ties[:n]):
        sig[k, :n_ch] = s
        y[:, k] = d
    return sig, y


def accumulate_np(sig, y):
    out = sig.copy()
    out[:, :y.shape[0]] = (sig[:, :y.shape[0]].astype(np.float64) + y.T).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------ copy segments
def reflect_index(q, n):
    """np.pad(.., 'reflect') as an index map of period 2 (n - 1) -- heal_reflect's formula"""
    q = np.asarray(q, dtype=np.int64)
    if n == 1:
        return np.zeros_like(q)
    P = 2 * (n - 1)
    q = np.mod(q, P)
    return np.where(q < n, q, P - q)


def padded_source_np(x, n_valid, n_padded, q):
    """fix_length(x, n_padded) under np.pad(.., A, 'reflect'), read at q + A -- by np.pad itself"""
    q = np.asarray(q, dtype=np.int64)
    base = np.concatenate((np.asarray(x[:n_valid], dtype=np.float32), np.zeros(max(0, n_padded - n_valid), np.float32)))[:n_padded]
    A = int(max(0, -q.min(initial=0), q.max(initial=0) - n_padded + 1))
    return np.pad(base, (A, A), "reflect")[q + A]


def padded_source_periodic(x, n_valid, n_padded, q):
    r = reflect_index(q, n_padded)
    x = np.asarray(x, dtype=np.float32)
    safe = np.minimum(r, max(len(x) - 1, 0))
    return np.where(r < n_valid, x[safe] if len(x) else np.float32(0), np.float32(0)).astype(np.float32)


class CopyCase:
    def __init__(self, name, src, src_start, dst_start, lens, dst_len, padded=False, n_valid=0, n_padded=0):
        self.name, self.src, self.padded, self.n_valid, self.n_padded, self.dst_len = name, src, padded, n_valid, n_padded, dst_len
        self.src_start, self.dst_start, self.lens = (np.asarray(a, dtype=np.int64) for a in (src_start, dst_start, lens))
        self.run_start = np.concatenate(([0], np.cumsum(self.lens)[:-1])).astype(np.int64)
        self.total = int(self.lens.sum())
        self.src.setflags(write=False)

    def __repr__(self):
        return self.name


SENTINEL = np.float32(-7.5e37)


def copy_segments_np(c, source=padded_source_np):
    """-> dst (dst_len,) float32: SENTINEL where no segment writes"""
    dst = np.full(c.dst_len, SENTINEL, dtype=np.float32)
    for s0, d0, ln in zip(c.src_start, c.dst_start, c.lens):
        q = s0 + np.arange(ln, dtype=np.int64)
        dst[d0:d0 + ln] = source(c.src, c.n_valid, c.n_padded, q) if c.padded else c.src[q]
    return dst


def _laid_out(name, lens, n_src=None, gap=3, seed=0, **kw):
    """segments of the given lengths read from random places of a random source, written `gap` samples apart"""
    rng = np.random.default_rng(seed + len(lens))
    lens = np.asarray(lens, dtype=np.int64)
    n_src = n_src or int(lens.max(initial=1)) + 50
    src = rng.standard_normal(n_src).astype(np.float32)
    src_start = [int(rng.integers(0, n_src - ln + 1)) for ln in lens]
    dst_start = np.concatenate(([gap], gap + np.cumsum(lens + gap)[:-1]))
    return CopyCase(name, src, src_start, dst_start, lens, int(lens.sum() + gap * (len(lens) + 1)), **kw)


def _padded(name, n_valid, n_padded, ranges, seed=9):
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(max(n_valid, 1)).astype(np.float32)
    lens = [b - a for a, b in ranges]
    dst_start = np.concatenate(([2], 2 + np.cumsum(np.asarray(lens) + 2)[:-1]))
    return CopyCase(name, src, [a for a, _ in ranges], dst_start, lens, int(sum(lens) + 2 * (len(lens) + 1)), padded=True,
                    n_valid=n_valid, n_padded=n_padded)


_COPY_BUILDERS = {
    "len_1_7_255": lambda: _laid_out("len_1_7_255", [1, 7, 255]),
    "forty_short": lambda: _laid_out("forty_short", [3 + (7 * k) % 58 for k in range(40)]),         # 40 segments, 1242 samples: one span
    "zero_lengths": lambda: _laid_out("zero_lengths", [0, 5, 0, 0, 300, 0, 9, 0, 0]),
    "straddle": lambda: _laid_out("straddle", [2000, 100, 3000, 10, 2100]),                           # 2000..2100 crosses 2048
    "short_then_span": lambda: _laid_out("short_then_span", [1] * 30 + [4200] + [2] * 25),
    "total2047": lambda: _laid_out("total2047", [1000, 1047]),
    "total2048": lambda: _laid_out("total2048", [1000, 1048]),
    "total2049": lambda: _laid_out("total2049", [1000, 1049]),
    "total1": lambda: _laid_out("total1", [1]),
    # padded mode: before sample 0, behind n_padded, the zeros of fix_length, all three in one range
    "pad_ends": lambda: _padded("pad_ends", 37, 50, [(-20, 5), (45, 70), (37, 50), (30, 40), (-49, 99), (0, 37)]),
    "pad_periods_valid3": lambda: _padded("pad_periods_valid3", 3, 5, [(-12, 17)]),
    "pad_periods_valid5": lambda: _padded("pad_periods_valid5", 5, 5, [(-12, 17), (-12, -11), (16, 17)]),
    "pad_n1": lambda: _padded("pad_n1", 1, 1, [(-3, 4), (0, 1)]),
    "pad_n1_empty": lambda: _padded("pad_n1_empty", 0, 1, [(-3, 4)]),
    "pad_n2": lambda: _padded("pad_n2", 2, 2, [(-7, 9)]),
}
COPY_CASES = tuple(_COPY_BUILDERS)


def copy_case(name):
    if ("copy", name) not in _cache:
        _cache["copy", name] = _COPY_BUILDERS[name]()
    return _cache["copy", name]
