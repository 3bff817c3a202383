"""Inputs that reach every cell of K_rsfix's filter tables one tap at a time, and the proof (run by test_fixed_rate_inputs_cpu.py, no
GPU) that the derived bound fixed_rate_np.tolerance notices a wrong cell on them.

Sweep shapes: rates 1023 -> 1024 and 1024 -> 1023 on 1100 samples.  The ideal phases are k / 1024 and k / 1023, so the table
offsets walk every row in half steps (eta about 0 or 0.5) and every (wing, table index) cell the tap-count rule allows is read
by an output whose wings are both whole (allowed_cells() == reached_cells()).

Impulse trains: x = 1 at every S-th sample from phase p, 0 elsewhere, S a power of two >= the longest window of the shape.  An
output's window then holds at most one impulse (single_impulse()), so an output is ONE interpolated weight, or an exact zero:
the bound (K + 5) 2^-24 B has B = |win_j| + |delta_j| of that tap alone and pins the weight to about 1.2e-6 of itself.  Over
the S phases every tap of every output is met alone.

What a wrong kernel would give on the trains is computed here from the float64 table (shift_margins, drop_margins,
eta_swap_margins, extra_tap): the change of the one weight an output consists of, over that output's tolerance."""
import numpy as np

import fixed_rate_np as F

SWEEP_N = 1100
UP = (1023, 1024)
DOWN = (1024, 1023)
SWEPT_Z = (5, 8, 15, 16)
NAN_Q = 550                       # the sample the locality tests poison: far from both ends, so only table-limited wings see it


def train_period(z):
    """A power of two >= the longest window (the largest uncut tap count, 2 z at most): 16 up to num_zeros 8, 32 at 15 and 16"""
    s = 1
    while s < 2 * z:
        s *= 2
    return s


_plans = {}


def plan(a, b, z, n=SWEEP_N):
    key = (a, b, z, n)
    if key not in _plans:
        _plans[key] = F.Plan(n, a, b, num_zeros=z)
    return _plans[key]


def train(n, S, p):
    x = np.zeros(n, dtype=np.float32)
    x[p::S] = 1.0
    return x


def single_impulse(pl, S):
    """True when no output's window holds two samples of the same residue mod S"""
    if pl.K.max() > S:
        return False
    key = pl.o * S + pl.i % S
    return len(np.unique(key)) == len(key)


def train_outputs(pl, S):
    """(Y, B): Y[p, o] the oracle's output o on train p, B[p, o] its bound's B.  Needs single_impulse: each entry is one tap's
    weight (times 1.0) or 0, so nothing is summed and the values are those of Plan.evaluate bit for bit."""
    n_out = pl.t1 - pl.t0
    Y = np.zeros((S, n_out))
    B = np.zeros((S, n_out))
    p = pl.i % S
    Y[p, pl.o] = pl.w
    B[p, pl.o] = pl.aw
    return Y, B


def allowed_cells(pl):
    """The (wing, table index) cells the tap-count rule (nwin - off) // step allows: the left offset is int(frac * P) with
    frac < scale, the right one int((scale - frac) * P) with 0 <= frac, so off <= int(scale * P) on the right and
    off < scale * P on the left."""
    nwin = F.P * pl.num_zeros + 1
    top = pl.scale * F.P
    cells = set()
    for wing, offs in ((0, range(0, int(np.ceil(top)))), (1, range(0, int(top) + 1))):
        for off in offs:
            for k in range((nwin - off) // pl.step):
                cells.add((wing, off + k * pl.step))
    return cells


def reached_cells(pl):
    """The cells read by outputs whose wings are both whole"""
    m = pl.whole[pl.o]
    return set(zip(pl.wing[m].tolist(), pl.j[m].tolist()))


def _tol_per_tap(pl):
    """The tolerance of the train output in which a tap stands alone"""
    return F.tolerance(pl.K[pl.o], pl.aw)


def _extended(pl):
    """win and delta with one zero entry behind the table (the `next offset` of the last entry)"""
    return np.append(pl.win, 0.0), np.append(pl.delta, 0.0)


def shift_margins(pl):
    """A row's cells replaced by the next offset's: tap j reads (win, delta)[j + 1].  -> {(wing, row): the largest change /
    tolerance over the outputs and taps of that row}"""
    win, delta = _extended(pl)
    wrong = win[pl.j + 1] + pl.eta * delta[pl.j + 1]
    margin = np.abs(wrong - pl.w) / _tol_per_tap(pl)
    rows = pl.off[pl.wing, pl.o]
    return _max_by(list(zip(pl.wing.tolist(), rows.tolist())), margin)


def drop_margins(pl):
    """A tap left out, or its sample index off by one (the train is 0 beside an impulse): the output loses the whole weight.
    -> {(wing, table index): the SMALLEST |weight| / tolerance over the outputs that read the cell}"""
    margin = np.abs(pl.w) / _tol_per_tap(pl)
    return {k: -v for k, v in _max_by(list(zip(pl.wing.tolist(), pl.j.tolist())), -margin).items()}


def eta_swap_margins(pl, min_gap):
    """The left wing interpolated with the right wing's eta and the other way round.  -> {(off_l, off_r): the largest change /
    tolerance over the outputs of that phase pair and their taps}, for the pairs whose etas differ by more than min_gap"""
    other = pl.eta_out[1 - pl.wing, pl.o]
    wrong = pl.win[pl.j] + other * pl.delta[pl.j]
    margin = np.abs(wrong - pl.w) / _tol_per_tap(pl)
    gap = np.abs(pl.eta_out[0] - pl.eta_out[1])[pl.o]
    keep = gap > min_gap
    pairs = list(zip(pl.off[0][pl.o][keep].tolist(), pl.off[1][pl.o][keep].tolist()))
    return _max_by(pairs, margin[keep])


def extra_tap(pl, S):
    """Tap number cnt taken although the rule ends the wing at cnt (`tap 7` of a row with off >= 2 at num_zeros 8): its table
    index off + cnt step is still inside the table for most rows, and holds a weight (entry N itself is an exact 0: skipped).
    -> {(wing, row): the largest |float32 weight| over the whole-wing outputs of that row whose extra sample exists and whose
    train output (the train through that sample) is an exact zero of the oracle}.  A kernel that takes the tap gives that
    weight where the test demands 0."""
    N = F.P * pl.num_zeros
    out = {}
    for wing in (0, 1):
        off, cnt = pl.off[wing], pl.cnt[wing]
        j = off + cnt * pl.step
        i = pl.n0 - cnt if wing == 0 else pl.n0 + cnt + 1
        ok = pl.whole & (j < N) & (i >= 0) & (i < pl.n)
        first, last = pl.n0 - pl.cnt[0] + 1, pl.n0 + pl.cnt[1]          # the window: the sample is outside, and S - 1 or
        ok &= (last - first + 1 < S)                                     # fewer samples wide, so the train misses it
        for m in np.nonzero(ok)[0]:
            w = np.float32(pl.win[j[m]]) + np.float32(pl.eta_out[wing, m]) * np.float32(pl.delta[j[m]])
            key = (wing, int(off[m]))
            out[key] = max(out.get(key, 0.0), abs(float(w)))
    return out


def extra_rows(pl):
    """The (wing, row) pairs of whole-wing outputs whose tap number cnt would still lie inside the table, below entry N"""
    N = F.P * pl.num_zeros
    rows = set()
    for wing in (0, 1):
        m = pl.whole & (pl.off[wing] + pl.cnt[wing] * pl.step < N)
        rows |= set((wing, int(r)) for r in pl.off[wing][m])
    return rows


def _max_by(keys, values):
    out = {}
    for k, v in zip(keys, values.tolist()):
        if k not in out or v > out[k]:
            out[k] = v
    return out


def nan_map(pl, q):
    """-> (hit, left, right): the outputs whose taps hold sample q, and those that hold it in the left / right wing"""
    n_out = pl.t1 - pl.t0
    left = np.zeros(n_out, dtype=bool)
    right = np.zeros(n_out, dtype=bool)
    m = pl.i == q
    left[pl.o[m & (pl.wing == 0)]] = True
    right[pl.o[m & (pl.wing == 1)]] = True
    return left | right, left, right


def just_outside(pl, q):
    """Outputs whose wing ends one sample short of q although the wing's row still has a table entry for it: distance cnt on the
    left (n0 - cnt == q) and cnt + 1 on the right (n0 + cnt + 1 == q), i.e. 7 and 8 at num_zeros 8 with off >= 2.
    -> (left outputs, right outputs)"""
    N = F.P * pl.num_zeros
    res = []
    for wing in (0, 1):
        cnt = pl.cnt[wing]
        i = pl.n0 - cnt if wing == 0 else pl.n0 + cnt + 1
        res.append(np.nonzero((i == q) & (pl.off[wing] + cnt * pl.step < N) & (pl.off[wing] >= 2))[0])
    return res
