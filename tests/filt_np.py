"""numpy float64 restatement of K_sosfiltfilt's blocked algorithm (csrc/filt.hip), and the exact block matrices.

sosfiltfilt_blocked does on the CPU what the kernels do, sum by sum (without fused multiply-adds, which the kernels may use):
odd extension; per direction and section the zero-state end state of every 256-sample block, the chain
s[b+1] = P s[b] + r[b] over the blocks -- one level, or two levels with Q over 256-block super-blocks -- and every block re-run
from its true state.  P and Q come from the library (par_sosfilt_block_matrices), so the restatement shows what the ALGORITHM
loses against the long-double oracle once the matrices are right; parent_matrices is the plain-double repeated squaring the
matrices were formed with before, kept for the record of what that lost."""
import ctypes
import fractions
import functools

import numpy as np

from filt_inputs import BLOCK, SUPER


def library_matrices(section):
    """(P, Q) of one section (b0 b1 b2 a0 a1 a2) as the library forms them: float64 [4] each, row-major"""
    from pyaudiorestoration_amd import _lib
    sec = np.ascontiguousarray(section, dtype=np.float64)
    P, Q = np.empty(4), np.empty(4)
    _lib.lib().par_sosfilt_block_matrices(sec.ctypes.data_as(ctypes.c_void_p), P.ctypes.data_as(ctypes.c_void_p),
                                          Q.ctypes.data_as(ctypes.c_void_p))
    return P, Q


def _mat_pow_double(a00, a01, a10, a11, e):
    p00, p01, p10, p11 = 1.0, 0.0, 0.0, 1.0
    while e > 0:
        if e & 1:
            p00, p01, p10, p11 = p00 * a00 + p01 * a10, p00 * a01 + p01 * a11, p10 * a00 + p11 * a10, p10 * a01 + p11 * a11
        a00, a01, a10, a11 = a00 * a00 + a01 * a10, a00 * a01 + a01 * a11, a10 * a00 + a11 * a10, a10 * a01 + a11 * a11
        e >>= 1
    return np.array([p00, p01, p10, p11])


def parent_matrices(section):
    """(P, Q) by repeated squaring in plain double, Q = P^256 of the rounded P: the arithmetic of the code before the fix"""
    a1, a2 = float(section[4]), float(section[5])
    P = _mat_pow_double(-a1, 1.0, -a2, 0.0, BLOCK)
    return P, _mat_pow_double(P[0], P[1], P[2], P[3], SUPER)


# ---- exact powers ---------------------------------------------------------------------------------------------------------------
def _dyadic(values):
    """floats -> (integers m_i, k) with values[i] = m_i / 2^k exactly"""
    ratios = [float(v).as_integer_ratio() for v in values]
    k = max(d.bit_length() - 1 for _, d in ratios)
    return [n * ((1 << k) // d) for n, d in ratios], k


def exact_power(m4, squarings):
    """M^(2^squarings) of the float64 2x2 matrix m4 (row-major), exactly: (integers [4], k) with entry i = integers[i] / 2^k.
    The entries of M are dyadic rationals, so every power is one too."""
    (a, b, c, d), k = _dyadic(m4)
    for _ in range(squarings):
        bc, tr = b * c, a + d
        a, b, c, d = a * a + bc, b * tr, c * tr, d * d + bc
        k *= 2
    return [a, b, c, d], k


def power_fixed(m4, squarings, bits=1024):
    """exact_power with every square cut to `bits` fractional bits: the 65536th power of a section's matrix has 7 10^6 bits and
    takes seconds, this takes a millisecond.  Each cut moves an entry by at most 2^-bits and a later squaring multiplies a
    perturbation by at most 2 max |entry| (< 2^15 on every cascade here), so after 16 squarings the result is within
    2^(240 - bits) of the exact power: 2^-784, against the 2^-53 it is compared at."""
    (a, b, c, d), k = _dyadic(m4)
    for _ in range(squarings):
        bc, tr = b * c, a + d
        a, b, c, d = a * a + bc, b * tr, c * tr, d * d + bc
        k *= 2
        if k > bits:
            a, b, c, d = (v >> (k - bits) if v >= 0 else -(-v >> (k - bits)) for v in (a, b, c, d))     # towards zero
            k = bits
    return [a, b, c, d], k


def matrix_error(got4, exact):
    """max |got - exact| / max |exact| over the four entries, in integer arithmetic.  Where the exact power lies below the
    smallest normal double (a wide band's A^65536) no double can hold it: the error is then taken relative to 2^-1022."""
    ints, k = exact
    shift = max(k, 1074)
    diff = 0
    for g, e in zip(got4, ints):
        n, d = float(g).as_integer_ratio()          # g = n / d, d a power of two <= 2^1074
        diff = max(diff, abs(n * ((1 << shift) // d) - (e << (shift - k))))
    scale = max(max(abs(e) for e in ints) << (shift - k), 1 << (shift - 1022))
    cut = max(0, scale.bit_length() - 256)              # (the quotient to 2^-200 or so: the integers can have 10^7 bits)
    return float(fractions.Fraction(diff >> cut, scale >> cut))


def section_matrix(section):
    return [-float(section[4]), 1.0, -float(section[5]), 0.0]


# ---- the blocked algorithm ------------------------------------------------------------------------------------------------------
def odd_ext(x, pad):
    return np.concatenate([2.0 * x[0] - x[pad:0:-1], x, 2.0 * x[-1] - x[-2:-pad - 2:-1]]) if pad else x.copy()


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker's product with Veltkamp's split; the kernels get e from one fused multiply-add)"""
    p = a * b
    ta, tb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ta - (ta - a), tb - (tb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _row(ph0, pl0, ph1, pl1, z0, z1, r):
    """(ph0 + pl0) z0 + (ph1 + pl1) z1 + r summed as if in twice the precision and rounded once: chain_row of filt.hip"""
    a, ae = _two_prod(ph0, z0)
    b, be = _two_prod(ph1, z1)
    s, se = _two_sum(a, b)
    t, te = _two_sum(s, r)
    return t + (((ae + be) + (pl0 * z0 + pl1 * z1)) + (se + te))


def _chain(P, z, r, keep):
    """walks s[b+1] = P s[b] + r[b] over the rows of r from the states z [m][2] (m chains side by side); keep: the start states.
    P = (head [4], tail [4]); tail None: the plain sums of the kernels before the chain was compensated"""
    hi, lo = P
    out = np.empty((z.shape[0], r.shape[1], 2)) if keep else None
    z0, z1 = z[:, 0].copy(), z[:, 1].copy()
    for b in range(r.shape[1]):
        if keep:
            out[:, b, 0], out[:, b, 1] = z0, z1
        if lo is None:
            z0, z1 = hi[0] * z0 + hi[1] * z1 + r[:, b, 0], hi[2] * z0 + hi[3] * z1 + r[:, b, 1]
        else:
            z0, z1 = (_row(hi[0], lo[0], hi[1], lo[1], z0, z1, r[:, b, 0]), _row(hi[2], lo[2], hi[3], lo[3], z0, z1, r[:, b, 1]))
    return out if keep else np.stack([z0, z1], axis=1)


def tails(section, P, Q):
    return _tails(tuple(float(v) for v in section), tuple(P), tuple(Q))


@functools.lru_cache(maxsize=None)
def _tails(section, P, Q):
    """the double nearest to (exact power - P) and (exact power - Q) per entry: what the kernels get as the low halves of the
    library's double-double powers (which agree with these to ~2^-100 of the largest entry)"""
    out = []
    for got, (ints, k) in ((P, exact_power(section_matrix(section), 8)), (Q, power_fixed(section_matrix(section), 16))):
        out.append(np.array([float(fractions.Fraction(e, 1 << k) - fractions.Fraction(float(g))) for g, e in zip(got, ints)]))
    return out


def _section_pass(u, sec, zi, first, two_level, matrices, compensated):
    """one section over the pass-ordered signal u [L] -> its output [L]"""
    b0, b1, b2, _, a1, a2 = (float(v) for v in sec)
    L = len(u)
    nblk = -(-L // BLOCK)
    ub = np.zeros(nblk * BLOCK)
    ub[:L] = u
    ub = ub.reshape(nblk, BLOCK)
    P, Q = matrices(sec)
    Pl, Ql = tails(sec, P, Q) if compensated else (None, None)
    P, Q = (P, Pl), (Q, Ql)

    def run(z0, z1, write):
        y = np.empty_like(ub) if write else None
        for t in range(BLOCK):
            xv = ub[:, t]
            yv = b0 * xv + z0
            z0 = b1 * xv - a1 * yv + z1
            z1 = b2 * xv - a2 * yv
            if write:
                y[:, t] = yv
        return y if write else np.stack([z0, z1], axis=1)
    r = run(np.zeros(nblk), np.zeros(nblk), False)            # the zeros behind L leave the last block's record unused
    start = np.array([[zi[0] * first, zi[1] * first]])
    if not two_level:
        s = _chain(P, start, r[None], True)[0]
    else:
        nsup = -(-nblk // SUPER)
        rp = np.zeros((nsup * SUPER, 2))
        rp[:nblk] = r
        rp = rp.reshape(nsup, SUPER, 2)
        # (the last super-block's own record is never read, so its padding does not matter)
        R = _chain(P, np.zeros((nsup, 2)), rp, False)
        S = _chain(Q, start, R[None], True)[0]
        s = _chain(P, S, rp, True).reshape(nsup * SUPER, 2)[:nblk]
    return run(s[:, 0].copy(), s[:, 1].copy(), True).reshape(-1)[:L]


def sosfiltfilt_blocked(sos, zi, x, padlen, two_level, matrices=library_matrices, compensated=True):
    """the kernels' arithmetic in numpy: sos [n_sections][6], zi = scipy.signal.sosfilt_zi(sos), two_level as the entry point
    chooses it (the single form from two super-blocks on, the batched form always)"""
    cur = odd_ext(np.asarray(x, dtype=np.float64), padlen)
    for direction in range(2):
        u = cur[::-1] if direction else cur
        first = u[0]
        for sec, z in zip(sos, zi):
            u = _section_pass(u, sec, z, first, two_level, matrices, compensated)
        cur = u[::-1] if direction else u
    return cur[padlen:len(cur) - padlen].copy()


def single_form_two_level(n, padlen):
    """par_sosfiltfilt_f64 walks one plain chain while the signal is one super-block long, the two-level chain from two on"""
    L = n + 2 * padlen
    return -(-(-(-L // BLOCK)) // SUPER) > 1
