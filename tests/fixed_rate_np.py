"""Float64 numpy statement of the fixed-ratio resampler (resampy 0.4: filter 'sinc_window' + interpn.resample_f with positions
t * (1 / ratio)), written from the algorithm and not from the kernel.  It also returns what the float32 error bound needs."""
import numpy as np
import scipy.signal

P = 512
ROLLOFF = 0.945


def table(num_zeros=8):
    """(win, delta): win[j] = hann_sym(2N + 1)[N + j] * rolloff * sinc(rolloff * j / P), j = 0..N = P * num_zeros;
    delta[j] = win[j + 1] - win[j], delta[N] = 0."""
    N = P * num_zeros
    taper = scipy.signal.get_window("hann", 2 * N + 1, fftbins=False)[N:]
    win = taper * (ROLLOFF * np.sinc(ROLLOFF * np.arange(N + 1) / P))
    delta = np.zeros(N + 1)
    delta[:-1] = np.diff(win)
    return win, delta


def out_len(n, sr_orig, sr_new):
    return int(n * sr_new / sr_orig)


def taps(t, n, sr_orig, sr_new, num_zeros=8):
    """Table indices and sample indices of output t: (j_left, i_left, eta_left, j_right, i_right, eta_right, scale)."""
    ratio = float(sr_new) / sr_orig
    scale = min(1.0, ratio)
    step = int(scale * P)
    inc = 1.0 / ratio
    nwin = P * num_zeros + 1
    tr = t * inc
    n0 = int(tr)
    frac = scale * (tr - n0)
    idx = frac * P
    off = int(idx)
    eta_l = idx - off
    i = np.arange(min(n0 + 1, (nwin - off) // step))
    jl, il = off + i * step, n0 - i
    frac = scale - frac
    idx = frac * P
    off = int(idx)
    eta_r = idx - off
    k = np.arange(max(0, min(n - n0 - 1, (nwin - off) // step)))
    jr, ir = off + k * step, n0 + k + 1
    return jl, il, eta_l, jr, ir, eta_r, scale


def uncut_count(t, sr_orig, sr_new, num_zeros=8):
    """Taps of output t when neither wing is cut by an end of the signal (the table alone limits them)."""
    jl, _, _, jr, _, _, _ = taps(t, 1 << 62, sr_orig, sr_new, num_zeros)
    ratio = float(sr_new) / sr_orig
    scale = min(1.0, ratio)
    tr = t * (1.0 / ratio)
    off = int(scale * (tr - int(tr)) * P)
    return (P * num_zeros + 1 - off) // int(scale * P) + len(jr)


def oracle(x, sr_orig, sr_new, t0=0, t1=None, num_zeros=8):
    """Outputs [t0, t1) of the resampled x (1-D) in float64 -> (y, K, B): K[t] the tap count, B[t] = sum over the taps of
    (|win_j| + |delta_j|) * |x_i| with the table as resampy scales it (times min(1, ratio))."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if t1 is None:
        t1 = out_len(n, sr_orig, sr_new)
    win, delta = table(num_zeros)
    scale = min(1.0, float(sr_new) / sr_orig)
    if scale < 1.0:                       # resampy scales the table, then differences it
        win = win * scale
        delta = np.zeros_like(win)
        delta[:-1] = np.diff(win)
    y = np.zeros(t1 - t0)
    K = np.zeros(t1 - t0, dtype=np.int64)
    B = np.zeros(t1 - t0)
    ax = np.abs(x)
    for t in range(t0, t1):
        jl, il, el, jr, ir, er, _ = taps(t, n, sr_orig, sr_new, num_zeros)
        y[t - t0] = np.sum((win[jl] + el * delta[jl]) * x[il]) + np.sum((win[jr] + er * delta[jr]) * x[ir])
        K[t - t0] = len(jl) + len(jr)
        B[t - t0] = np.sum((np.abs(win[jl]) + np.abs(delta[jl])) * ax[il]) + np.sum((np.abs(win[jr]) + np.abs(delta[jr])) * ax[ir])
    return y, K, B


class Plan:
    """The taps of outputs [t0, t1) of one shape, taken once and kept: evaluate(x) is oracle(x, ...) for any x of length n, bit
    for bit (the same expressions on the same index arrays).  The taps are also kept flat, one entry per (output, wing, tap):
    o (output - t0), wing (0 left, 1 right), k (tap number in its wing), j (table index), i (sample index), eta, and per
    output n0, off[wing], cnt[wing] (taps the table allows) and whole (neither wing is cut by an end of the signal)."""

    def __init__(self, n, sr_orig, sr_new, t0=0, t1=None, num_zeros=8):
        if t1 is None:
            t1 = out_len(n, sr_orig, sr_new)
        self.n, self.t0, self.t1, self.num_zeros = n, t0, t1, num_zeros
        ratio = float(sr_new) / sr_orig
        self.scale = scale = min(1.0, ratio)
        self.step = step = int(scale * P)
        inc = 1.0 / ratio
        nwin = P * num_zeros + 1
        tr = np.arange(t0, t1) * inc                       # taps(), on every output at once
        n0 = tr.astype(np.int64)
        frac = scale * (tr - n0)
        idx_l = frac * P
        off_l = idx_l.astype(np.int64)
        idx_r = (scale - frac) * P
        off_r = idx_r.astype(np.int64)
        self.n0 = n0
        self.off = np.stack([off_l, off_r])
        self.eta_out = np.stack([idx_l - off_l, idx_r - off_r])
        self.cnt = (nwin - self.off) // step
        cut = np.stack([np.minimum(n0 + 1, self.cnt[0]), np.maximum(0, np.minimum(n - n0 - 1, self.cnt[1]))])
        self.whole = (n0 >= self.cnt[0]) & (n0 + self.cnt[1] + 1 < n)
        self.K = cut[0] + cut[1]
        win, delta = table(num_zeros)
        if scale < 1.0:
            win = win * scale
            delta = np.zeros_like(win)
            delta[:-1] = np.diff(win)
        self.win, self.delta = win, delta
        total = int(self.K.sum())
        self.o = np.repeat(np.arange(t1 - t0), self.K)
        self.wing = np.zeros(total, dtype=np.int64)
        self.k = np.zeros(total, dtype=np.int64)
        start = np.cumsum(self.K) - self.K
        for m in range(t1 - t0):
            s, cl, cr = start[m], cut[0, m], cut[1, m]
            self.k[s:s + cl] = np.arange(cl)
            self.k[s + cl:s + cl + cr] = np.arange(cr)
            self.wing[s + cl:s + cl + cr] = 1
        self.j = self.off[self.wing, self.o] + self.k * step
        self.i = np.where(self.wing == 0, n0[self.o] - self.k, n0[self.o] + self.k + 1)
        self.eta = self.eta_out[self.wing, self.o]
        self.w = win[self.j] + self.eta * delta[self.j]
        self.aw = np.abs(win[self.j]) + np.abs(delta[self.j])
        self._split = [(start[m], start[m] + cut[0, m], start[m] + self.K[m]) for m in range(t1 - t0)]

    def evaluate(self, x):
        """-> (y, K, B) as oracle(x, sr_orig, sr_new, t0, t1, num_zeros)"""
        x = np.asarray(x, dtype=np.float64)
        assert x.shape == (self.n,)
        ax = np.abs(x)
        y = np.zeros(self.t1 - self.t0)
        B = np.zeros(self.t1 - self.t0)
        w, aw, i = self.w, self.aw, self.i
        for m, (s, mid, e) in enumerate(self._split):
            y[m] = np.sum(w[s:mid] * x[i[s:mid]]) + np.sum(w[mid:e] * x[i[mid:e]])
            B[m] = np.sum(aw[s:mid] * ax[i[s:mid]]) + np.sum(aw[mid:e] * ax[i[mid:e]])
        return y, self.K.copy(), B


def tolerance(K, B):
    """Per output: the table entries, eta, eta * delta, the weight, its product with x and the scale multiply round once each
    in float32, and a float32 sum of K terms in any order adds at most (K - 1) * 2^-24 relative: (K + 5) * 2^-24 * B."""
    return (K + 5) * 2.0 ** -24 * B
