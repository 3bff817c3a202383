"""Inputs of tests/test_maxmono_gpu.py, and the restated launch geometry of par_maxmono_stft_f32 (csrc/stft.hip, MaxMonoGeom).
numpy only; tests/test_maxmono_cpu.py proves on the CPU what the GPU tests assume of these inputs."""
import collections

import numpy as np

INF32 = np.float32(np.inf)
SELECT_GRID_ROWS = 4096           # k_select_spectrum's grid rows: more frames take a second pass of its frame loop
SENTINEL = np.float32(-7777.25)   # cells no kernel may write
SPEC_SENTINEL = np.complex64(1e3 + 1e3j)

Spectra = collections.namedtuple("Spectra", "L R cls")      # cls: 0 tie, 1 |R| an ulp under |L|, 2 an ulp over, -1 free


def _normal_c64(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def tie_spectra(frames=7, bins=1031, seed=17):
    """L random; R = (+-float32|L|, 0) (or its nextafter down / up) so that np.abs(R) is exactly that float32: every bin of row 0
    a tie, the other rows tie / ulp-under / ulp-over by (frame + bin) % 3.  Odd bins in every other column carry R on the
    imaginary axis instead, and the sign alternates."""
    rng = np.random.default_rng(seed)
    L = _normal_c64(rng, (frames, bins))
    m = np.abs(L)
    assert m.dtype == np.float32
    f, b = np.indices((frames, bins))
    cls = (f + b) % 3
    cls[0] = 0
    mag = np.where(cls == 0, m, np.where(cls == 1, np.nextafter(m, -INF32), np.nextafter(m, INF32))).astype(np.float32)
    sign = np.where(b % 2 == 0, np.float32(1), np.float32(-1))
    on_imag = (b % 4) >= 2
    R = np.where(on_imag, 1j * (sign * mag), sign * mag).astype(np.complex64)
    return Spectra(L, R, cls)


def free_spectra(frames, bins, seed):
    """two independent random spectra (either side louder in about half the cells)"""
    rng = np.random.default_rng(seed)
    return Spectra(_normal_c64(rng, (frames, bins)), _normal_c64(rng, (frames, bins)), np.full((frames, bins), -1))


# parts of the special-value spectra: every pair (re, im) of these is a cell of L, and of R
NAN_A = np.array([0x7fc00123], dtype=np.uint32).view(np.float32)[0]         # quiet NaNs with payloads
NAN_B = np.array([0xffc00001], dtype=np.uint32).view(np.float32)[0]
DENORM = np.float32(3e-42)
PARTS = (INF32, -INF32, NAN_A, NAN_B, np.float32(-0.0), np.float32(0.0), DENORM, -DENORM, np.float32(1.5), np.float32(-1.5))


def special_spectra():
    """(P^2, P^2) cells: row = L's (re, im) pair, column = R's, over all pairs of PARTS"""
    p = np.array(PARTS, dtype=np.float32)
    re, im = np.meshgrid(p, p, indexing="ij")
    cell = np.empty(re.size, dtype=np.complex64)
    cell.real, cell.imag = re.reshape(-1), im.reshape(-1)
    L = np.repeat(cell[:, None], len(cell), axis=1)
    R = np.repeat(cell[None, :], len(cell), axis=0)
    return Spectra(np.ascontiguousarray(L), np.ascontiguousarray(R), np.full(L.shape, -1))


def is_denormal(a):
    a = np.abs(np.asarray(a, dtype=np.float32))
    return (a > 0) & (a < np.finfo(np.float32).tiny)


def bits(a):
    """the cells' bit patterns: uint32 of float32, uint64 of complex64 (one word per cell)"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ fused geometry, restated
LDS_LIMIT = 160 * 1024


def frames_per_round(n_fft):
    return max(1, 4096 // n_fft)                                   # 256 threads / (n_fft / 16 lanes per frame); one frame from 4096 on


def frame_lds_bytes(n_fft):
    h = n_fft // 2
    return frames_per_round(n_fft) * (h + h // 8 + 8) * 8


def lds_bytes(n_fft, hop):
    ring = n_fft + frames_per_round(n_fft) * hop
    return frame_lds_bytes(n_fft) + (2 * ring + hop) * 4


def supported(n_fft, hop):
    return 16 <= n_fft <= 8192 and n_fft & (n_fft - 1) == 0 and 1 <= hop <= n_fft and lds_bytes(n_fft, hop) <= LDS_LIMIT


def largest_fused_hop(n_fft):
    return max(h for h in range(1, n_fft + 1) if supported(n_fft, h))


def run_samples(n_fft, hop):
    """samples of the padded signal one workgroup owns"""
    s = -(-n_fft // hop)
    fr = frames_per_round(n_fft)
    rounds = -(-12 * s // fr)
    return (fr * rounds - (s - 1)) * hop


def runs(n, n_fft, hop):
    return -(-(n + n_fft // 2) // run_samples(n_fft, hop))


# (n_fft, hop): every compiled variant at hop n_fft / 4, hop 1, hop = n_fft, a hop that does not divide, the largest fused hop
FUSED_SIZES = tuple((1 << k, (1 << k) // 4) for k in range(4, 14)) + ((16, 1), (64, 64), (512, 96), (8192, largest_fused_hop(8192)))


def lengths(n_fft, hop):
    """shorter than a reflection; one run; 25 n_fft + 1; and, where that is fewer than three runs, three runs with a ragged end"""
    out = [max(1, n_fft // 2 - 3), max(n_fft, min(run_samples(n_fft, hop) - n_fft // 2, 3 * n_fft) - 1), 25 * n_fft + 1]
    if runs(out[-1], n_fft, hop) < 3:
        out.append(2 * run_samples(n_fft, hop) + n_fft + 1)
    return out


def stereo(n, seed):
    """(n, 2) float32: two takes of one programme (tones under an envelope, plus independent noise), the second delayed and 2 dB
    down -- either channel is the louder one in about half the bins"""
    rng = np.random.default_rng(seed)
    t = np.arange(n + 37, dtype=np.float64)
    prog = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in ((0.3, 0.0113, 0.1), (0.2, 0.0517, 1.0), (0.1, 0.1931, 2.0), (0.05, 0.3707, 0.5)))
    prog = prog * (0.6 + 0.4 * np.sin(2 * np.pi * t / 997.0)) + 0.05 * rng.standard_normal(n + 37)
    x = np.stack([prog[37:], 0.8 * prog[:n]], axis=1) + 0.02 * rng.standard_normal((n, 2))
    return x.astype(np.float32)
