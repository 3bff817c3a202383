"""Inputs of tests/test_sinc_nt_gpu.py -- K_sinc's generic tap loops (taps_unity / taps_general, csrc/sinc_block.h) across the tap
count NT -- and what tests/test_sinc_nt_inputs_cpu.py verifies of them without a GPU.  Nothing here touches the library.

NT_SET is written out; test_sinc_nt_inputs_cpu.py derives every entry that depends on the tap-mode table (csrc/sinc_tap_modes.h)
from the table program and asserts that it is listed.

A case is (regime, variant): a float64 position array `p0 + cumsum(period)` and the input length it needs.  Which lanes, waves
and tiles of k_sinc_pos it reaches is restated here from the positions alone (classify): place_from_pos and the span rule of
sinc_tile_body.

Where the construction has to depart from the plainest reading of a regime's or a signal's name:
 * `low`: the kernel reads the period as the DIFFERENCE of two positions, so "the next double above 8" is built into the
   positions (every difference is 8 plus one ulp of the position); a full tile at period 8 spans 8184 input samples and is never
   staged, so these cases are one partial tile of 360 outputs.
 * `nyquist`: where every lane of a regime has fc < 1 the Nyquist tone lies in the stop band and the output is 1e-4 .. 1e-7 of
   the input -- no 1e-5 of ITS peak means anything in float32 (nor does the reference's own float32 output carry it).  There the
   tone is laid over the case's unit noise, which supplies the scale; the tone's alternating signs are still the worst case for
   the cancelling tap sums.  Regimes with fc = 1 lanes pass the tone and take it alone.
 * NaN footprints: an output is poisoned when its window [ind - NT, ind + NT - 1] holds the sample; that is 2 NT outputs at
   period 1 and 2 NT / period otherwise."""
import numpy as np

TILE, BLOCK, WAVE, CAP, CHUNK = 1024, 256, 64, 4096, 4
N_OUT = 3 * TILE + 328          # three full tiles and a partial one

NT_SMALL = (1, 2, 3, 4)                               # a single LAST chunk in the reciprocal form, all four masks
NT_TAYLOR = (5, 6, 7, 8, 9, 12, 13)                   # the first polynomial rows
NT_FIRST_LINEAR, NT_FIRST_CONSTANT = 6, 5             # smallest NT at which a chunk runs in that form
NT_LAST_LINEAR = (6, 10, 11, 12, 15, 16)              # every NT whose LAST chunk is linear (residues 2, 2, 3, 0, 3, 0; none has 1)
NT_LAST_CONSTANT = (20, 5, 14, 19)                    # the smallest NT of each residue 0..3 whose LAST chunk is constant
NT_NEXT_TO_SPECIALISED = (31, 33, 49, 51)
NT_SPECIALISED = (32, 50)
NT_LARGE = (64, 80, 100, 101, 102, 103, 128, 200, 256)
# a fused mono wave stages mx - mn + 2 (NT + 5) <= 1024 samples for its 256 outputs: 379 is the largest NT that fits at speed 1,
# 378 still fits and 382 no longer does on every curve within 1 % of it
NT_FUSED_SPAN = (378, 379, 380, 382)
NT_TOP = (511, 512)
NT_SET = tuple(sorted(set(NT_SMALL + NT_TAYLOR + NT_LAST_LINEAR + NT_LAST_CONSTANT + NT_NEXT_TO_SPECIALISED + NT_SPECIALISED +
                          NT_LARGE + NT_FUSED_SPAN + NT_TOP)))
NT_NONFINITE = (1, 2, 3, 4, 5, 6, 7, 8, 31, 33, 100, 101, 102, 103, 512)
NT_FUSED = (3, 7, 33, 100, 200) + NT_FUSED_SPAN + (512,)

GENTLE_FC = (0.9995, 0.995, 0.99, 0.985, 0.97)
STEEP_FC = (0.9, 0.6, 0.45, 0.2, 0.13)
SIGNALS = ("noise", "cutoff", "nyquist", "impulses")
PHI = 0.4


def _rng(regime, variant, NT, salt):
    # (str hashes are salted per process: spell the names out as numbers)
    return np.random.default_rng([sum(ord(ch) * (i + 1) for i, ch in enumerate(regime)), int(round(float(variant) * 1e6)), NT, salt])


def variants(regime):
    return {"unity": (0,), "gentle": GENTLE_FC, "gentle_edge": (0,), "steep": STEEP_FC, "mixed": (0,), "low": (0, 1), "lead": (0,),
            "tail": (0,), "wide": (0, 1)}[regime]


REGIMES = ("unity", "gentle", "gentle_edge", "steep", "mixed", "low", "lead", "tail", "wide")
CASES = tuple((r, v) for r in REGIMES for v in variants(r))


def wide_period(NT, over):
    """period at which a full tile's span 1023 * period + 2 (NT + 4) lands ~6 samples under / over the 4096 that are staged"""
    return (CAP - 2 * (NT + CHUNK) + (6 if over else -6)) / (TILE - 1)


def positions(regime, variant, NT):
    """(float64 positions, len_in, the fc a cutoff tone of the regime takes)"""
    rng = _rng(regime, variant, NT, 1)
    start = float(NT + 40) + 0.3                                    # clear of the leading edge unless the regime is about it
    n_out = N_OUT
    len_in = None
    if regime == "unity":
        n_int = 2 * NT + 90                                          # exact integers: shift 0 -> 1e-20 (and room for a whole NaN footprint)
        per = np.concatenate((np.ones(n_int), [0.5], np.ones(99), [0.75], 0.97 + 0.03 * rng.random(n_out)))[:n_out]
        pos = float(NT + 40) + np.concatenate(([0.0], np.cumsum(per[:-1])))
        fc = 1.0
    elif regime in ("gentle", "steep"):
        fc = float(variant)
        if fc < 0.34:                                                # a full tile spans 1023 / fc input samples: staged, with 2 (NT + 4)
            n_out = 360                                              # more, up to fc = 0.334 at NT = 512; below, one partial tile
        pos = start + np.cumsum(np.full(n_out, 1.0 / fc))
    elif regime == "gentle_edge":                                    # dd = 1/32 at period 32/31, crossed in the second tile
        per = np.linspace(32 / 31 - 0.004, 32 / 31 + 0.004, n_out)
        pos = start + np.cumsum(per)
        fc = float(1.0 / np.median(per))
    elif regime == "mixed":
        per = np.where(np.arange(n_out) % 2 == 0, 0.99, 1.01)
        pos = start + np.cumsum(per)
        fc = 1.0 / 1.01
    elif regime == "low":
        n_out = 360
        pos = np.empty(n_out)
        pos[0] = float(NT + 40) + 0.3125                             # (exact sums: every difference is 8.0 to the bit)
        for i in range(1, n_out):
            pos[i] = pos[i - 1] + 8.0
            if variant:
                pos[i] = np.nextafter(pos[i], np.inf)
        fc = 0.125
    elif regime == "lead":                                           # ind < NT: the reference's mis-aligned taps
        per = 0.97 + 0.03 * rng.random(n_out)
        pos = 0.3 + np.concatenate(([0.0], np.cumsum(per[:-1])))
        fc = 1.0
    elif regime == "tail":                                           # the window clipped by min(ind + NT, len_in)
        per = 0.97 + 0.03 * rng.random(n_out)
        pos = start + np.cumsum(per)
        len_in = int(np.ceil(pos[-1])) + 1
        pos += (len_in - 1) - pos[-1]                                # the last position IS len_in - 1
        fc = 1.0
    elif regime == "wide":
        n_out = 2 * TILE + 328
        fc = 1.0 / wide_period(NT, bool(variant))
        pos = start + np.cumsum(np.full(n_out, 1.0 / fc))
    else:
        raise KeyError(regime)
    if len_in is None:
        len_in = int(np.ceil(pos[-1])) + NT + 12
    return np.ascontiguousarray(pos, dtype=np.float64), len_in, fc


NYQUIST_PASSES = ("unity", "mixed", "lead", "tail")                 # regimes with fc = 1 lanes


def signal(name, regime, variant, NT, len_in, fc, pos):
    n = np.arange(len_in, dtype=np.float64)
    noise = _rng(regime, variant, NT, 2).uniform(-1.0, 1.0, len_in)
    if name == "noise":
        x = noise
    elif name == "cutoff":
        # phi: in phase with the first position.  At a constant period 1 / fc every output sees the tone at the same phase,
        # and the output, 0.5 cos(pi fc p + phi), is as small as that phase makes it
        x = np.cos(np.pi * fc * (n - pos[0])) if fc < 1.0 else np.cos(np.pi * n + PHI)
    elif name == "nyquist":
        x = np.cos(np.pi * n + PHI)
        if regime not in NYQUIST_PASSES:
            x = x + noise
    elif name == "impulses":
        # 2 NT + 50 apart and more: an output reads at most one of them, so exactly one tap weight.  Each is put under an
        # output's window at a tap offset that cycles through -NT .. NT - 1 (where the read head skips input, a fixed grid
        # of impulses would be missed)
        x = np.zeros(len_in)
        ind = np.rint(pos).astype(np.int64)
        last, t = -(1 << 40), 0
        for j in range(len(pos)):
            site = int(ind[j]) + (3 * t) % (2 * NT) - NT
            if site >= last + 2 * NT + 50 and 0 <= site < len_in:
                x[site] = 1.0
                last, t = site, t + 1
    else:
        raise KeyError(name)
    return x.astype(np.float32)


def case_signal(name, regime, variant, NT):
    """(positions, signal) of one case"""
    pos, len_in, fc = positions(regime, variant, NT)
    return pos, signal(name, regime, variant, NT, len_in, fc, pos)


def nonfinite_output(regime, NT, n_out):
    return NT + 45 if regime == "unity" else n_out // 2 - 100


def nonfinite_signal(kind, regime, variant, NT, pos, len_in):
    """unit noise with one NaN or +inf sample under the middle of the positions (`unity`: of the run of exact integers, where the
    period is 1 and the footprint 2 NT outputs); returns (signal, index)"""
    x = signal("noise", regime, variant, NT, len_in, 1.0, pos)
    at = int(np.rint(pos[nonfinite_output(regime, NT, len(pos))]))
    x[at] = {"nan": np.nan, "inf": np.inf}[kind]
    return x, at


def footprint(pos, NT, len_in, at):
    """outputs whose window signal[max(ind - NT, 0) : min(ind + NT, len_in)] holds sample `at`"""
    ind = np.rint(pos).astype(np.int64)
    return (np.maximum(ind - NT, 0) <= at) & (at < np.minimum(ind + NT, len_in))


NONFINITE_CASES = (("unity", 0), ("gentle", 0.9995), ("steep", 0.6))


def periods(pos):
    dp = np.empty(len(pos))
    dp[:-1] = pos[1:] - pos[:-1]
    dp[-1] = dp[-2]                                                  # the last output reuses the previous period
    return dp


def classify(pos, NT, len_in):
    """What k_sinc_pos makes of the positions, from place_from_pos and sinc_tile_body: counts of lanes, waves and tiles per path"""
    dp = periods(pos)
    ind = np.rint(pos).astype(np.int64)
    one, low, lead = ~(dp > 1.0), dp > 8.0, ind < NT
    dd = np.where(one, 0.0, (dp - 1.0) / np.maximum(dp, 1e-12))
    out = dict(n=len(pos), fc1=int(one.sum()), fc_lt1=int((~one).sum()), low=int(low.sum()), lead=int(lead.sum()),
               clipped=int((ind + NT > len_in).sum()), integer=int((pos == ind).sum()), half=int((np.abs(pos - ind) == 0.5).sum()),
               staged=0, unstaged=0, fast=0, slow=0, waves_unity=0, waves_mixed=0, groups_gentle=0, groups_steep=0, groups_edge=0)
    for j0 in range(0, len(pos), TILE):
        sl = slice(j0, min(j0 + TILE, len(pos)))
        anchor = int(np.rint(pos[j0])) & ~1
        c = np.rint(pos[sl] - anchor).astype(np.int64)
        span = int(c.max() - c.min()) + 2 * (NT + CHUNK)
        staged = span <= CAP
        out["staged" if staged else "unstaged"] += 1
        fast = staged & ~lead[sl] & ~low[sl]
        out["fast"] += int(fast.sum())
        out["slow"] += int((~fast).sum())
        # thread t owns outputs j0 + t + 256 r, r = 0..3; its wave is t // 64; the generic fc < 1 loop takes rows (0, 1) and (2, 3)
        k = np.arange(sl.stop - sl.start)
        wave, row = (k % BLOCK) // WAVE, k // BLOCK
        for w in range(BLOCK // WAVE):
            m = wave == w
            if not (m & fast).any():
                continue
            u = one[sl][m]
            if u.all():
                out["waves_unity"] += 1
                continue
            out["waves_mixed"] += int(u.any())
            for pair in (0, 1):
                g = m & (row // 2 == pair)
                if not g.any():                                     # (a pair of rows past the end: runs on idle lanes)
                    continue
                hi = dd[sl][g].max()
                out["groups_edge" if abs(hi - 0.03125) < 1e-6 else "groups_gentle" if hi < 0.03125 else "groups_steep"] += 1
    return out


def sinc_f64(pos, sig, NT, reverse=False, every=1):
    """The reference's sum in float64, output not rounded to float32, taps added first to last or last to first; of every
    `every`-th output"""
    p = np.asarray(pos, dtype=np.float64)
    sig = np.asarray(sig)
    len_in = len(sig)
    N = np.arange(-NT, NT, dtype=np.float64)
    win = np.hanning(2 * NT + 1).astype(np.float32)[:2 * NT].astype(np.float64)
    fc = np.minimum(1.0 / np.maximum(1e-12, periods(p)), 1.0)[::every]
    p = p[::every]
    ind = np.rint(p).astype(np.int64)
    lower, upper = np.maximum(0, ind - NT), np.minimum(ind + NT, len_in)
    idx = lower[:, None] + np.arange(2 * NT)[None, :]
    taps = np.where(idx < upper[:, None], sig[np.minimum(idx, len_in - 1)].astype(np.float64), 0.0)
    terms = taps * (np.sinc((N[None, :] - (p - ind)[:, None]) * fc[:, None]) * fc[:, None]) * win[None, :]
    if reverse:
        terms = terms[:, ::-1]
    return np.cumsum(terms, axis=1)[:, -1]


# ---- the fused form: speed curves, about N_OUT outputs each ----------------------------------------------------------------------
FUSED_CURVES = ("c0.99", "c1.01", "sine", "c0.3")


def fused_curve(name, NT):
    """(sampletimes, speeds, len_in): N_OUT outputs and the taps behind the last one"""
    mean = {"c0.99": 0.99, "c1.01": 1.01, "sine": 1.0, "c0.3": 0.3}[name]
    len_in = int(N_OUT / mean) + 40
    m = 41
    st = np.linspace(0.0, float(len_in), m)
    sp = np.full(m, mean)
    if name == "sine":
        sp = 1.0 + 0.02 * np.sin(np.arange(m) * 0.9)
    return st, sp, len_in


def fused_usable_waves(pos, NT, outputs_per_wave=256, capw=1024):
    """(usable, all) waves of the mono fused kernel: a wave stages rint(last) - rint(first) + 2 (NT + 5) samples, at most capw"""
    ind = np.rint(pos).astype(np.int64)
    ok = [int(ind[min(a + outputs_per_wave, len(pos)) - 1] - ind[a]) + 2 * (NT + CHUNK + 1) <= capw
          for a in range(0, len(pos), outputs_per_wave)]
    return sum(ok), len(ok)


# ---- the constant form's first row, as the device shows it --------------------------------------------------------------------------
PROBE_SHIFT = 0.125


def boundary_probe(NT):
    """(positions, impulse train, row read by each output or -1): period exactly 1 at a shift of 1/8, so every output near an
    impulse reads ONE tap weight sin(pi s) / pi * (n -+ s) * R_n(q) at q = 1/64, and every row n is read on both sides"""
    pos = float(NT + 40) + PROBE_SHIFT + np.arange(N_OUT, dtype=np.float64)
    len_in = int(pos[-1]) + NT + 12
    sig = signal("impulses", "unity", 0, NT, len_in, 1.0, pos)
    ind = np.rint(pos).astype(np.int64)
    row = np.full(len(pos), -1)
    for site in np.flatnonzero(sig):
        near = (ind - NT <= site) & (site < ind + NT)
        row[near] = np.abs(site - ind[near])
    return pos, sig, row


def constant_form_signature(n, q=PROBE_SHIFT ** 2):
    """relative error of R_n(q) = K / (n^2 - q) when the row holds the mid-range constant K (1 / n^2 + 1 / (n^2 - 1/4)) / 2"""
    n2 = np.asarray(n, dtype=np.float64) ** 2
    return 0.5 * (1.0 / n2 + 1.0 / (n2 - 0.25)) * (n2 - q) - 1.0
