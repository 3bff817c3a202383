"""Inputs and oracles that pin K_gauge (par_gauge_offset_f32) at the C ABI (tests/test_gauge_kernels_gpu.py; proofs in
tests/test_gauge_inputs_cpu.py; derivations in NOTES.md "Renoiser: the offset gauge").  No GPU and no library here.

Integer inputs.  x holds integers in [-4, 4], h_re and h_im integers in [-8, 8], all float32.  With n_fft <= 2050 every partial sum
of a tap chain is an integer below 2050 * 32 < 2^24, so every FMA is exact and z(i, j) is the same integer in any summation order;
sum z and sum |z|^2 stay below 2^53, so the kernel's compensated sums and its tree are exact as well.  What is left to round are
the last lines of k_gauge_final, and the oracle is exact: z as an int64 product over gauge_np.padded / frames_of (the reference's
definition, nothing of the kernel's geometry), S and S2 as Python integers, var = S2 / F - |S|^2 / F^2 as a Fraction.

The tolerance, on squares:   |got^2 - var| <= VAR_ROUNDINGS * 2^-53 * S2 / F.   With u = 2^-53 and V = S2 / F >= |S|^2 / F^2
(Cauchy-Schwarz), the last lines of k_gauge_final compute, from the exact S_re, S_im, S2 and F,
    d = fl(S2 / F)                                   1 rounding:            |d - V| <= u V
    mr = fl(S_re / F), mi = fl(S_im / F)             1 rounding each, squared below: 2 u on each part of |S|^2 / F^2
    c = fl(fl(mr mr) + fl(mi mi))                    1 u on each part for its square, 1 u for the sum
                                                     |c - |S|^2 / F^2| <= 4 u |S|^2 / F^2 <= 4 u V
    var' = fl(d - c)                                 1 rounding of a value of at most V: together |var' - var| <= 6 u V
    got = fl(sqrt(max(0, var')))                     1 rounding (the clamp only moves var' towards var >= 0); got^2 carries it twice
which is 1 + 2 + 1 + 1 + 1 + 2 = 8 first-order terms, each at most u V; the second-order terms are below 2^-49 of that."""
import functools
from fractions import Fraction

import numpy as np

import gauge_np as G

TILE, BLOCK, CHUNK, TAP_BLOCK = 2048, 256, 1024, 16      # kGaTile, kGaBlock, kGaChunk, kGaTapBlock of csrc/gauge.hip
VAR_ROUNDINGS = 8
U64 = Fraction(1, 2 ** 53)

# name -> shapes (n_fft, hop, n): the smallest that reach each path (test_gauge_inputs_cpu.py proves that they do)
SHAPES = {
    "rotation": ((50, 7, 5000),),
    "slots_stride": ((64, 300, 5000),),
    "hop_over_tile": ((64, 2500, 7000), (64, 2049, 9000)),
    "final_runs": ((16, 7, 526341), (16, 4, 614400)),
    "chunk_tail": ((1030, 9, 4500), (2050, 48, 6000)),
    "no_dense": ((2050, 5, 40), (16, 4, 1)),
    "tile_seam": ((2, 3, 2047), (2, 3, 2048), (2, 3, 2049)),
    "odd": ((51, 4, 203), (51, 7, 5000), (3, 2, 5), (3, 5000, 4097)),
    "existing": tuple(G.GPU_SHAPES.values()) + (G.IMPULSE_SHAPE,),
}
DELTA_GROUPS = ("rotation", "chunk_tail", "hop_over_tile", "odd")
REAL_SHAPES = ("small", "not_pow2_hop_not_dividing", "default_chunks_and_tiles")


def shapes_of(*groups):
    return [s for g in groups for s in SHAPES[g]]


ALL_SHAPES = shapes_of(*SHAPES)
MULTI_WG_SHAPES = [s for s in ALL_SHAPES if s[2] + s[0] // 2 - s[0] + 1 > TILE]


def shape_id(shape):
    return "-".join(str(v) for v in shape)


# ---------------------------------------------------------------------------------------------------------------- inputs

# shape -> seed offset where the first seeds missed a precondition of test_gauge_inputs_cpu.py: (16, 4, 1) is ONE sample, var >= S2 / (2 F)
# on its four pads is then a property of the filter alone, which seeds 0 and 1 do not have
RESEED = {(16, 4, 1): 2}


def _seed(shape, salt):
    n_fft, hop, n = shape
    return [salt + 100 * RESEED.get(shape, 0), n_fft, hop, n]


def int_signal(shape):
    """Integers in [-4, 4], the first and last sample not 0 (the one real sample the right reflection holds is x[n - 1]).  Where a
    pad has fewer than 8 frames the draw is one hop of values repeated with alternating sign, x[t + hop] = -x[t]: consecutive frames
    of a pad then cancel in the mean, which keeps var >= S2 / (2 F) on pads of two to five frames, where no seed of independent
    values does on all of several thousand pads."""
    n_fft, hop, n = shape
    r = np.random.default_rng(_seed(shape, 11))
    if (n + n_fft) // hop + 1 < 8:
        t = np.arange(n)
        x = r.integers(-4, 5, min(n, hop))[t % hop] * np.where((t // hop) % 2 == 0, 1, -1)
    else:
        x = r.integers(-4, 5, n)
    for k, v in ((0, 3), (n - 1, -3)):
        if x[k] == 0:
            x[k] = v
    return x.astype(np.float32)


def int_filter(shape):
    """(h_re, h_im), integers in [-8, 8] without 0: every tap weighs in both parts"""
    r = np.random.default_rng(_seed(shape, 12))
    h = r.integers(1, 9, (2, shape[0])) * r.choice([-1, 1], (2, shape[0]))
    return h[0].astype(np.float32), h[1].astype(np.float32)


def delta_signal(shape):
    """integers in [-4, 4]; the first and last two samples are distinct values of magnitude 3 and 4, so that the two reflections
    and the first and last real sample cannot be taken for each other"""
    n = shape[2]
    assert n >= 4
    x = np.random.default_rng(_seed(shape, 13)).integers(-4, 5, n).astype(np.float32)
    x[0], x[1], x[n - 2], x[n - 1] = 3.0, -4.0, 4.0, -3.0
    return x


def delta_taps(n_fft):
    ms = {0, 7, 8, 15, 16, n_fft - 2, n_fft - 1}
    if n_fft > 1024:
        ms |= {1023, 1024, 1039, 1040}
    return sorted(m for m in ms if 0 <= m < n_fft)


def delta_filter(n_fft, m, part):
    """(h_re, h_im) = e_m in the real part (part 0) or in the imaginary part (part 1)"""
    h = np.zeros((2, n_fft), dtype=np.float32)
    h[part, m] = 1.0
    return h[0], h[1]


# ----------------------------------------------------------------------------------------------------------- exact oracle

def frames(n, n_fft, hop, i):
    """the reference's frame count for pad i: the padded signal has n + i + 3 (n_fft // 2) samples"""
    return (n + i + 3 * (n_fft // 2) - n_fft) // hop + 1


def padded_int(x, i, n_fft, zero_left=False, zero_right=False):
    """gauge_np.padded as int64; zero_left / zero_right blank a reflection (the mutations of the power test)"""
    p = G.padded(x, i, n_fft)
    q = p.astype(np.int64)
    assert np.array_equal(q, p)
    half = n_fft // 2
    if zero_left:
        q[:half] = 0
    if zero_right:
        q[len(q) - half:] = 0
    return q


def exact_z(x, h_re, h_im, n_fft, hop, i, js=None, **blank):
    """(z_re, z_im) of pad i as int64, every frame or the frames js"""
    fr = G.frames_of(padded_int(x, i, n_fft, **blank), n_fft, hop)
    if js is not None:
        fr = fr[js]
    return fr @ np.asarray(h_re).astype(np.int64), fr @ np.asarray(h_im).astype(np.int64)


def moments(zr, zi):
    """(S_re, S_im, S2, F) as Python integers"""
    zr, zi = np.asarray(zr, dtype=np.int64), np.asarray(zi, dtype=np.int64)
    assert float(np.abs(zr).sum()) + float(np.abs(zi).sum()) < 2.0 ** 52 and float((zr * zr + zi * zi).sum()) < 2.0 ** 53
    return int(zr.sum()), int(zi.sum()), int((zr * zr + zi * zi).sum()), len(zr)


def variance(m):
    sr, si, s2, F = m
    return Fraction(s2, F) - Fraction(sr * sr + si * si, F * F)


def tolerance(m):
    return VAR_ROUNDINGS * U64 * Fraction(m[2], m[3])


def error_over_bound(got, m):
    """|got^2 - var| / tolerance for one pad (a Fraction; inf where the tolerance is 0 and got is not)"""
    if not np.isfinite(got):
        return float("inf")
    err, tol = abs(Fraction(float(got)) ** 2 - variance(m)), tolerance(m)
    return float(err / tol) if tol else (0.0 if err == 0 else float("inf"))


class IntCase:
    """One integer shape with its exact z per pad (int64, read-only) and moments; computed once per process"""

    def __init__(self, shape, x, h_re, h_im):
        self.shape, self.x, self.h_re, self.h_im = shape, x, h_re, h_im
        n_fft, hop, n = shape
        self.z = []
        for i in range(hop):
            zr, zi = exact_z(x, h_re, h_im, n_fft, hop, i)
            zr.setflags(write=False), zi.setflags(write=False)
            self.z.append((zr, zi))
        self.moments = [moments(zr, zi) for zr, zi in self.z]
        for a in (x, h_re, h_im):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def int_case(shape):
    return IntCase(shape, int_signal(shape), *int_filter(shape))


@functools.lru_cache(maxsize=None)
def delta_moments(shape):
    """(x, {(m, part): [moments per pad]}) for the delta filters: z(i, j) = p_i[j hop + m], straight from the padded signal"""
    n_fft, hop, n = shape
    x = delta_signal(shape)
    x.setflags(write=False)
    out = {(m, part): [] for m in delta_taps(n_fft) for part in (0, 1)}
    for i in range(hop):
        p = padded_int(x, i, n_fft)
        F = (len(p) - n_fft) // hop + 1
        for m in delta_taps(n_fft):
            z = p[m::hop][:F]
            assert len(z) == F
            zero = np.zeros_like(z)
            out[(m, 0)].append(moments(z, zero))
            out[(m, 1)].append(moments(zero, z))
    return x, out


# ------------------------------------------------------------------------------- exact float32 FMA chain for real filters

def fma_chain(P, h, repair=True):
    """acc = fma(P[m], h[m], acc) over ascending m in float32, column by column of P (n_fft, rows; float64 holding float32
    values) -> (acc float32, steps repaired, smallest non-zero |acc| met).  The product of two float32 is exact in float64; s =
    acc + product rounds to 53 bits and TwoSum gives its error e exactly.  float32(s) is the FMA's result unless s lies exactly
    halfway between two float32 and e != 0: then the true sum lies on e's side of the midpoint, and the tie is broken that way
    (repair=False keeps the double rounding of gauge_np.emulate_f32)."""
    acc = np.zeros(P.shape[1], dtype=np.float32)
    repaired, smallest = 0, np.inf
    inf32 = np.float32(np.inf)
    for m in range(P.shape[0]):
        a = acc.astype(np.float64)
        pr = P[m] * h[m]
        s = a + pr
        r = s.astype(np.float32)
        if repair:
            bb = s - a
            e = (a - (s - bb)) + (pr - bb)                        # TwoSum: a + pr = s + e exactly
            r64 = r.astype(np.float64)
            up, dn = np.nextafter(r, inf32), np.nextafter(r, -inf32)
            go_up = (e > 0) & (s > r64) & (s == 0.5 * (r64 + up.astype(np.float64)))
            go_dn = (e < 0) & (s < r64) & (s == 0.5 * (r64 + dn.astype(np.float64)))
            repaired += int(np.count_nonzero(go_up) + np.count_nonzero(go_dn))
            r = np.where(go_up, up, np.where(go_dn, dn, r))
        acc = r
        nz = np.abs(acc[acc != 0])
        if nz.size:
            smallest = min(smallest, float(nz.min()))
    return acc, repaired, smallest


def emulate_chain(x, h32_re, h32_im, n_fft, hop, repair=True):
    """z of every pad as the kernel computes it, bit for bit: ([(z_re, z_im) float32 per pad], steps repaired, smallest non-zero
    partial sum)"""
    hr = np.asarray(h32_re, dtype=np.float32).astype(np.float64)
    hi = np.asarray(h32_im, dtype=np.float32).astype(np.float64)
    z, repaired, smallest = [], 0, np.inf
    per = max(1, 4096 // max(1, (len(x) + n_fft) // hop + 1))          # pads per batch
    for i0 in range(0, hop, per):
        blocks = [G.frames_of(G.padded(x, i, n_fft), n_fft, hop) for i in range(i0, min(hop, i0 + per))]
        P = np.ascontiguousarray(np.concatenate(blocks).T)
        re, k_re, s_re = fma_chain(P, hr, repair)
        im, k_im, s_im = fma_chain(P, hi, repair)
        repaired, smallest = repaired + k_re + k_im, min(smallest, s_re, s_im)
        at = 0
        for b in blocks:
            z.append((re[at:at + len(b)], im[at:at + len(b)]))
            at += len(b)
    return z, repaired, smallest


@functools.lru_cache(maxsize=None)
def real_case(name):
    """(x, h_re, h_im, z per pad, steps repaired, smallest partial sum) for gauge_np.GPU_SHAPES[name]: noise_and_tone through
    renoiser.gauge_filter rounded to float32, z by the exact chain"""
    from pyaudiorestoration_amd import renoiser
    n_fft, hop, n = G.GPU_SHAPES[name]
    x = G.noise_and_tone(n)
    h = renoiser.gauge_filter(G.SR, n_fft, G.BAND)
    hr, hi = h.real.astype(np.float32), h.imag.astype(np.float32)
    z, repaired, smallest = emulate_chain(x, hr, hi, n_fft, hop)
    for a in (x, hr, hi) + tuple(v for p in z for v in p):
        a.setflags(write=False)
    return x, hr, hi, z, repaired, smallest


def float_moments(zr, zi):
    """(S_re, S_im, S2, F) of float32 z, exact, as Fractions"""
    fr = [Fraction(float(v)) for v in zr]
    fi = [Fraction(float(v)) for v in zi]
    return sum(fr), sum(fi), sum(a * a + b * b for a, b in zip(fr, fi)), len(fr)


def std_naive(zr, zi):
    """gauge_np.emulate_f32's last lines"""
    zr, zi = zr.astype(np.float64), zi.astype(np.float64)
    F = len(zr)
    var = np.sum(zr * zr + zi * zi) / F - ((np.sum(zr) / F) ** 2 + (np.sum(zi) / F) ** 2)
    return np.sqrt(max(0.0, var))


# --------------------------------------------------------------------------------------------------------- geometry replay

class Geometry:
    """ga_geometry, ga_j_lo / ga_j_hi, ga_edge_frame and k_gauge_final's walk over the partials, replayed"""

    def __init__(self, n_fft, hop, n):
        self.n_fft, self.hop, self.n, self.half = n_fft, hop, n, n_fft // 2
        self.dense = max(0, n + self.half - n_fft + 1)
        self.n_wg = -(-self.dense // TILE)
        self.slots = min(hop, TILE)
        if self.dense > 0:
            self.edges = (self.half + hop - 1) // hop + 1 + (n_fft - self.half) // hop + 2
        else:
            self.edges = (n + hop - 1 + self.half) // hop + 1
        self.per = -(-self.n_wg // BLOCK)
        self.chunks = [min(CHUNK, n_fft - c0) for c0 in range(0, n_fft, CHUNK)]

    def frames(self, i):
        return frames(self.n, self.n_fft, self.hop, i)

    def j_lo(self, i):
        return (self.half + i + self.hop - 1) // self.hop

    def j_hi(self, i):
        return (self.dense - 1 + self.half + i) // self.hop if self.dense > 0 else -1

    def edge_frame(self, i, e):
        j_lo, j_hi = self.j_lo(i), self.j_hi(i)
        j = e if j_lo > j_hi or e < j_lo else j_hi + 1 + (e - j_lo)
        return j if j < self.frames(i) else -1

    def lane_runs(self):
        """[(first workgroup, end) per lane of k_gauge_final]"""
        return [(th * self.per, min((th + 1) * self.per, self.n_wg)) for th in range(BLOCK)]

    def rotation(self, w):
        return (w * TILE) % self.hop

    def slot(self, i, w):
        """the slot of workgroup w that k_gauge_final reads for pad i (it skips one >= slots)"""
        res = (-(self.half + i)) % self.hop
        return (res - self.rotation(w)) % self.hop

    def dense_t(self, i):
        """every t that k_gauge_final's walk sums for pad i: partial[w][slot] holds t = w TILE + slot + k hop below the
        workgroup's valid count"""
        ts = []
        for lo, hi in self.lane_runs():
            for w in range(lo, hi):
                c = self.slot(i, w)
                if c >= self.slots:
                    continue
                valid = min(TILE, self.dense - w * TILE)
                ts.append(w * TILE + np.arange(c, valid, self.hop, dtype=np.int64))
        return np.concatenate(ts) if ts else np.zeros(0, dtype=np.int64)

    def frame_sources(self, i):
        """frame number of everything the kernel sums for pad i, dense first: (frames of the dense t, frames of the edge lanes)"""
        t = self.dense_t(i)
        assert np.all((t + self.half + i) % self.hop == 0)
        edge = [self.edge_frame(i, e) for e in range(self.edges)]
        return (t + self.half + i) // self.hop, np.array([j for j in edge if j >= 0], dtype=np.int64)

    def covers_every_frame_once(self, i):
        dense_j, edge_j = self.frame_sources(i)
        every = np.sort(np.concatenate((dense_j, edge_j)))
        return len(every) == self.frames(i) and np.array_equal(every, np.arange(self.frames(i)))

    def covers_by_count(self, i):
        """the same statement from the ranges alone (for sweeps): dense frames are j_lo .. j_hi, the edge lanes enumerate
        0 .. j_lo - 1 and j_hi + 1 .. in order, so the cover is exact when there are lanes enough"""
        j_lo, j_hi, F = self.j_lo(i), self.j_hi(i), self.frames(i)
        if j_lo > j_hi:
            return self.edges >= F
        return j_hi < F and self.edges >= j_lo + (F - 1 - j_hi)

    def workgroup_of(self, i, j):
        """dense workgroup of frame j of pad i (array), -1 for an edge frame"""
        j = np.asarray(j, dtype=np.int64)
        t = j * self.hop - self.half - i
        return np.where((j >= self.j_lo(i)) & (j <= self.j_hi(i)), t // TILE, -1)
