"""Speed curves that take the rare rungs of the plan's retry ladder (plan_impl in csrc/pos.hip), and a host restatement of the
ladder's decisions.

plan_impl makes a plan in "goes": after each one it reads the header back and either settles or goes again -- lazy, eager, eager with
the chunked cumsum of the long segments, any of them with host-made lengths, and behind them the serial host path.  CASES names one
curve per rung (and per pair of rungs that a real curve can take together); predict() says, from the curve alone, which goes the
ladder makes and what the ABI and the header then show.  It restates the decisions, not the arithmetic: lengths in exact rational
arithmetic, positions by the reference's own numpy loop.  tests/test_plan_ladder_cpu.py holds predict() against the literal
expectation of every case and proves the case's preconditions; tests/test_plan_ladder_gpu.py holds the library against both.

Constants of csrc/pos_plan.h and csrc/pos.hip, by value (as tests/xcorr_inputs.py restates xc_fft_len):"""
from fractions import Fraction

import numpy as np

K_LAZY_MAX_N = 1024            # kLazyMaxN: most outputs of a lazy plan's segment; also the first go's n_in / (m - 1) bound
K_LONG_SEG = 32768             # kLongSeg: longer segments take the chunked cumsum (they need checkpoint slots that fit)
K_MAX_DIRECT = 2048            # kMaxDirect: steps of the offset chain the stitch can take one by one
K_CK = 8                       # kCk: a cumsum checkpoint every 8 steps
K_TILE = 1024                  # kSincTileOutputs
TIE_ZONE = Fraction(1, 1 << 32)   # round_fixed: a cumulative length within 2^-32 of k + 1/2 is a near-tie
A_MIN, A_MAX = 2.0 ** -11, 2.0 ** 62   # want_fixed: a_i outside [2^-11, 2^62) raises kFlagRange (and counts as 0)
FLAG_AMBIGUOUS, FLAG_BAD_LENGTH, FLAG_RANGE, FLAG_VERIFY, FLAG_DIRECT_OVERFLOW, FLAG_CK_OVERFLOW, FLAG_CAP_AMBIGUOUS = 1, 2, 4, 8, 16, 32, 64
FORCE_EAGER = 8                # kForceEager
# header words (int32 view of PlanHeader) the GPU test reads, as _plan_arrays of tests/test_hip_parity.py returns them
H_CAP, H_FLAGS, H_N_DIRECT, H_N_LONG, H_LAZY, H_LAZY_FAIL = 8, 11, 12, 22, 26, 27


def fused_ck_len(max_out, m):
    return max_out // K_CK + m + 16


def fused_tiles(max_out):
    return max_out // K_TILE + 4


def default_max_out(st, sp):
    """resampling.fused_max_out"""
    return int(float(np.mean(sp)) * float(st[-1] - st[0]) * 1.01) + int(float(np.diff(st).max()) * float(sp.max())) + 1024


def lazy_segment_ok(n, s0, s1):
    lo, hi = min(s0, s1), max(s0, s1)
    return 2 <= n <= K_LAZY_MAX_N and lo >= 0.0625 and hi <= 64.0 and (hi - lo) <= 2.0 ** -9 * lo


def products(st, sp):
    """a_i = period_i * mean speed_i in the reference's float64 order (util/resampling.py:103, :111)"""
    return np.diff(st) * ((sp[:-1] + sp[1:]) / 2.0)


def exact_lengths(a):
    """The device scan: cumulative a_i in exact arithmetic (products outside the range count as 0), each rounded to nearest, a sum ON
    k + 1/2 downwards (round_fixed).  -> (seg_start [m], near-ties, least distance of a sum that is no near-tie from the zone)"""
    start, run, ties, margin = [0], Fraction(0), 0, None
    for v in a:
        if A_MIN <= v < A_MAX:
            run += Fraction(float(v))
        whole = run.numerator // run.denominator
        d = abs(run - whole - Fraction(1, 2))
        if d < TIE_ZONE:
            ties += 1
        else:
            margin = d - TIE_ZONE if margin is None else min(margin, d - TIE_ZONE)
        start.append(whole + (1 if run - whole > Fraction(1, 2) else 0))
    return np.array(start, dtype=np.int64), ties, (float(margin) if margin is not None else None)


def host_lengths(a):
    """The reference's recurrence (:111-118; host_lengths in pos.hip).  -> seg_start [m], or None where the library's refuses"""
    start, err = [0], 0.0
    for v in a:
        inerr = float(v) + err
        n = round(inerr)
        if not 0 <= n < 9.0e15:
            return None
        err = inerr - n
        start.append(start[-1] + n)
    return np.array(start, dtype=np.int64)


def replay(st, sp, n_in, start):
    """The reference's loop on given lengths, with numpy's own arithmetic: the offset in front of every segment it can build (it stops
    in front of one with n < 2) and the one behind the last, the trim segment and the output length.  Goes on behind the trim, as
    the device does."""
    off, x = [], float(st[0])
    trim_seg, len_out, bad, trim_min = None, None, None, None
    for i in range(len(sp) - 1):
        n = int(start[i + 1] - start[i])
        if n < 2:
            bad = i
            break
        off.append(x)
        seg = np.cumsum(1 / (np.arange(n) / (n - 1) * (sp[i + 1] - sp[i]) + sp[i])) + x
        if trim_seg is None and seg[0] <= n_in <= seg[-1]:
            d = np.abs(seg - n_in)
            trim_seg, len_out = i, int(start[i]) + int(np.argmin(d))
            trim_min = (float(d.min()), int(np.sum(d == d.min())))        # the least distance and how many positions have it
        x = float(seg[-1])
    if trim_seg is None and bad is None:
        len_out = int(start[-1])
    return np.array(off + [x]), trim_seg, len_out, bad, trim_min


def direct_steps(x):
    """Steps of the offset chain that off_element does not vouch for: offset <= 0 (`nonpos`), or the step's two ends not provably in one
    binade (`crossing`: within 2^-30 of a power of two counts)"""
    nonpos = int(np.sum(x[:-1] <= 0.0))
    pos = x[:-1] > 0.0
    lo, hi = 1.0 - 2.0 ** -30, 1.0 + 2.0 ** -30
    with np.errstate(invalid="ignore", divide="ignore"):
        e = [np.floor(np.log2(np.abs(v))) for v in (x[:-1] * lo, x[:-1] * hi, x[1:] * lo, x[1:] * hi)]
    crossing = int(np.sum(pos & ~((e[0] == e[1]) & (e[1] == e[2]) & (e[2] == e[3]))))
    return nonpos, crossing


def predict(st, sp, n_in, fused=True, eager=False, max_out=None, force_host=0):
    """The ladder of plan_impl for this call.  -> dict: goes (names of the device goes in order, "serial" last where it is taken),
    raises, path, flags (par_last_plan_flags), fused_ok, lazy, n_long, cap, len_out, trimmed -- and what the decisions hung on:
    ties, tie_margin, lazy_segments_ok, n_long_segments, nonpos, crossing, cap_dist, cap_thr, first_bad, trim_seg, trim_min (the
    least |position - n_in| in the trim segment and how many positions have it), lengths_agree (exact scan == host recurrence)."""
    st, sp = np.asarray(st, dtype=np.float64), np.asarray(sp, dtype=np.float64)
    m = len(sp)
    a = products(st, sp)
    if fused and max_out is None:
        max_out = default_max_out(st, sp)
    ck_len, max_tiles = (fused_ck_len(max_out, m), fused_tiles(max_out)) if fused else (0, 0)
    dev_start, ties, tie_margin = exact_lengths(a)
    host_start = host_lengths(a)
    in_range = bool(np.all((a >= A_MIN) & (a < A_MAX)))
    guess = (float(np.sum(sp.astype(np.longdouble))) / m) * float(st[-1] - st[0]) * 1.01      # trim_body, with an accurate sum
    cap_dist, cap_thr = abs(guess - round(guess)), abs(guess) * 1e-14 + 1e-12
    cap = int(np.mean(sp) * (st[-1] - st[0]) * 1.01)                                           # what the host settles: numpy's order
    out = dict(ties=ties, tie_margin=tie_margin, cap_dist=cap_dist, cap_thr=cap_thr, cap=cap, in_range=in_range,
               lengths_agree=host_start is not None and bool(np.array_equal(dev_start, host_start)))

    def is_long(start, i):
        n = int(start[i + 1] - start[i])
        return fused and n > K_LONG_SEG and int(start[i]) // K_CK + i + (n + K_CK - 1) // K_CK <= ck_len

    def ck_fit(start, len_out):
        """k_tile_seg: the tile tables hold the plan, and every segment that starts in front of len_out has its checkpoint slots"""
        if (len_out + K_TILE - 1) // K_TILE + 1 > max_tiles:
            return False
        n = np.diff(start)
        need = (n > 0) & (start[:-1] < len_out)
        slots = start[:-1] // K_CK + np.arange(m - 1) + (n + K_CK - 1) // K_CK
        return bool(np.all(slots[need] <= ck_len))

    def device_go(start, lazy):
        """flags of a go that is not void, and what it found"""
        off, trim_seg, len_out, bad, trim_min = replay(st, sp, n_in, start)
        short = np.nonzero(np.diff(start) < 2)[0]
        first_bad = int(short[0]) if len(short) else None
        flags = 0 if in_range else FLAG_RANGE
        if first_bad is not None and not (trim_seg is not None and trim_seg < first_bad):
            flags |= FLAG_BAD_LENGTH
        nonpos, crossing = direct_steps(off)
        if nonpos + crossing > K_MAX_DIRECT:
            flags |= FLAG_DIRECT_OVERFLOW
        if cap_dist <= cap_thr:
            flags |= FLAG_CAP_AMBIGUOUS
        out.update(first_bad=first_bad, trim_seg=trim_seg, nonpos=nonpos, crossing=crossing, trim_min=trim_min)
        return flags, len_out, trim_seg is not None

    goes, last_flags = [], 0
    serial = bool(force_host & 3)
    lazy = fused and not serial and not eager and not (force_host & FORCE_EAGER) and n_in // (m - 1) <= K_LAZY_MAX_N
    with_long = host = False
    start, len_out, trimmed = dev_start, None, None
    while not serial:
        goes.append(("lazy" if lazy else "eager") + ("+long" if with_long else "") + ("+host" if host else ""))
        if host:
            if host_start is None:
                serial = True
                break
            start = host_start
        n = np.diff(start)
        seg_ok = [lazy_segment_ok(int(n[i]), sp[i], sp[i + 1]) for i in range(m - 1)]
        n_long_segments = sum(is_long(start, i) for i in range(m - 1))
        out.update(lazy_segments_ok=all(seg_ok), n_long_segments=n_long_segments)
        if lazy and not all(seg_ok):
            lazy = False                         # lazy_fail 1 (more than kMaxCand candidates, lazy_fail 2, is not restated: no case has them)
            continue
        if not lazy and n_long_segments and not with_long:
            with_long = True                     # lazy_fail 4
            continue
        flags, len_out, trimmed = device_go(start, lazy)
        if host is False and ties:
            flags |= FLAG_AMBIGUOUS
        last_flags |= flags
        flags &= ~FLAG_CAP_AMBIGUOUS             # settled on the side
        if flags == 0:
            break
        if flags == FLAG_AMBIGUOUS and not host:
            host = True
        else:
            serial = True
    out.update(goes=goes, raises=False)
    if serial:
        goes.append("serial")
        if host_start is None:
            out.update(raises=True)
            return out
        start = host_start
        off, trim_seg, len_out, bad, trim_min = replay(st, sp, n_in, start)
        out.update(trim_seg=trim_seg, trim_min=trim_min)
        if bad is not None and trim_seg is None:
            out.update(raises=True, bad_segment=bad)
            return out
        trimmed = trim_seg is not None
        if trimmed:                              # host_plan gives the segments behind the trim empty entries
            start = start.copy()
            start[trim_seg + 2:] = start[trim_seg + 1]
        n_long = sum(is_long(start, i) for i in range(m - 1))
        fused_ok = int(fused and ck_fit(start, len_out))
        out.update(path=1, lazy=False, n_long=n_long if fused else 0)
    else:
        fused_ok = 0 if not fused else (2 if lazy else 1) * int(ck_fit(start, len_out) if not lazy
                                                                  else (len_out + K_TILE - 1) // K_TILE + 1 <= max_tiles)
        out.update(path=2 if host else 0, lazy=bool(lazy and fused_ok), n_long=out["n_long_segments"] if with_long else 0)
    out.update(flags=last_flags, fused_ok=fused_ok, len_out=len_out, trimmed=trimmed, max_out=max_out)
    return out


# ------------------------------------------------------------------------------------------------------------------- the cases

def _gentle(m):
    return 1.0 + 0.01 * np.sin(0.013 * np.arange(m))


def _cap_curve():
    """the curve of test_buffer_bound_ambiguity_is_settled_with_numpys_order (tests/test_hip_parity.py)"""
    m, n = 400, 100000
    return np.linspace(0, n, m), np.full(m, 100500 / (n * 1.01)), n


def _range_curve(at, gap=0.0):
    st = np.linspace(0.0, 2e5, 201)
    st[at + 1] = st[at] + gap
    return st, np.ones(201), 100000


def _trim_curve(st0=1000.25, n_in=200000):
    return st0 + np.arange(2000) * 256.0, np.full(2000, 2.0), n_in


_TIES = np.arange(3000) * 256.5
_MIXED = np.concatenate(([0.0], np.cumsum([256.5] * 31 + [40000.0] + [256.5] * 32)))
_SPARSE_RAMP = (np.array([0.0, 120000.0, 300007.0]), np.array([1.0, 0.9, 1.07]), 280000)
_TRIM_SPARSE = (np.array([1000.25, 3000000.25]), np.array([2.0, 2.0]), 1000000)
HALF = "half"            # max_out = len_out // 2 (the GPU test and the CPU test put the oracle's length in)


class Case:
    """st, sp, n_in: the curve.  kwargs: what speed_plan_dev(fused=True) is called with besides.  Expectation of that call: goes, path,
    flags (par_last_plan_flags, exactly), fused_ok, n_long; raises: the reference and the library refuse the curve.  len_out: the
    oracle's length where it was recorded when the case was written (the CPU test holds the oracle to it).  spot: an output index the resampled signal is looked at around
    (None: the trim's end is the last of oracle_spot's windows anyway).  plain: expectation (goes, path, flags) of the entry without
    an aux buffer, where the test takes it too.  also: flag bits that may stand beside `flags` (see direct-overflow)."""

    def __init__(self, name, curve, goes, path, flags, fused_ok, n_long=0, kwargs=None, raises=False, len_out=None, spot=None,
                 plain=None, also=0):
        self.name, (self.st, self.sp, self.n_in) = name, curve
        self.st, self.sp = np.asarray(self.st, dtype=np.float64), np.asarray(self.sp, dtype=np.float64)
        self.goes, self.path, self.flags, self.fused_ok, self.n_long = goes, path, flags, fused_ok, n_long
        self.kwargs, self.raises, self.len_out, self.spot, self.plain, self.also = kwargs or {}, raises, len_out, spot, plain, also

    def call_kwargs(self, len_out):
        kw = dict(self.kwargs)
        if kw.get("max_out") == HALF:
            kw["max_out"] = len_out // 2
        return kw

    def predict(self, len_out=None):
        if len_out is None and self.kwargs.get("max_out") == HALF:
            len_out = predict(self.st, self.sp, self.n_in)["len_out"]
        kw = self.call_kwargs(len_out)
        return predict(self.st, self.sp, self.n_in, fused=True, eager=bool(kw.get("eager")), max_out=kw.get("max_out"),
                       force_host=int(kw.get("force_host_chain", 0)))

    def predict_plain(self):
        return predict(self.st, self.sp, self.n_in, fused=False, eager=True)


def _cases():
    st4000 = np.arange(4000) * 256.0
    lazy_plain = (st4000, _gentle(4000), int(0.97 * st4000[-1]))
    ties = (_TIES, np.ones(3000), int(0.97 * _TIES[-1]))
    ties2001 = np.arange(2001) * 256.5
    neg = lambda st0: (st0 + np.arange(4000) * 256.0, _gentle(4000), 300000)
    C = Case
    return [
        C("lazy-plain", lazy_plain, ["lazy"], 0, 0, 2),
        C("lazy-length-ties", ties, ["lazy", "lazy+host"], 2, 1, 2, len_out=746165, plain=(["eager", "eager+host"], 2, 1)),
        # (with periods of 256.5 the scan's lengths -- a sum ON the tie goes down -- are the recurrence's all the same: round() sends
        # 256.5 to the even 256; with 257.5 it sends it up to 258 and every pair of lengths differs from the scan's)
        C("lazy-length-ties-odd", (np.arange(3000) * 257.5, np.ones(3000), int(0.97 * 2999 * 257.5)), ["lazy", "lazy+host"], 2, 1, 2),
        C("eager-length-ties", ties, ["eager", "eager+host"], 2, 1, 1, kwargs=dict(eager=True), len_out=746165),
        C("mixed-long-length-ties", (_MIXED, np.ones(65), int(0.97 * _MIXED[-1])), ["lazy", "eager", "eager+long", "eager+long+host"],
          2, 1, 1, n_long=1, len_out=54473, spot=32 * 256),
        C("sparse-length-tie", (np.array([0.0, 100000.5, 250000.0]), np.ones(3), 240000), ["eager", "eager+long", "eager+long+host"],
          2, 65, 1, n_long=2, len_out=239999),      # (1.0 * 250000 * 1.01 is the integer 252500: 64 beside the 1)
        C("cap-ambiguous-lazy", _cap_curve(), ["lazy"], 0, 64, 2),
        C("cap-ambiguous-and-ties", (ties2001, np.ones(2001), int(0.97 * ties2001[-1])), ["lazy", "lazy+host"], 2, 65, 2),
        # (1.0 * 2e5 * 1.01 is the integer 202000: these three curves raise 64 beside their own flag)
        C("range-behind-trim", _range_curve(149), ["lazy", "eager", "serial"], 1, 4 | 64, 1, len_out=99999,
          plain=(["eager", "serial"], 1, 4 | 64)),
        C("range-behind-trim-1e-4", _range_curve(149, 1e-4), ["lazy", "eager", "serial"], 1, 4 | 64, 1, len_out=99999),
        C("range-in-front", _range_curve(49), ["lazy", "eager", "serial"], None, None, None, raises=True),
        # (a stitch that lost steps leaves offsets outside the binade their run vouches for: the verification of that same go may raise
        # 8 beside the 16, depending on which steps the table's atomic counter turned away)
        C("direct-overflow", neg(-600000.0), ["lazy", "serial"], 1, 16, 1, len_out=900225, spot="zero",
          plain=(["eager", "serial"], 1, 16), also=FLAG_VERIFY),
        C("direct-many", neg(-400000.0), ["lazy"], 0, 0, 2, len_out=700304, spot="zero", plain=(["eager"], 0, 0)),
        C("trim-tie-dense", _trim_curve(), ["lazy"], 0, 0, 2, len_out=397998, plain=(["eager"], 0, 0)),
        C("trim-tie-dense-eager", _trim_curve(), ["eager"], 0, 0, 1, kwargs=dict(eager=True), len_out=397998),
        # (2.0 * 2999000 * 1.01 is within 1e-9 of the integer 6057980: this curve raises 64; the next one does not)
        C("trim-tie-sparse", _TRIM_SPARSE, ["eager", "eager+long"], 0, 64, 1, n_long=1, len_out=1997998),
        C("trim-tie-sparse-plain-cap", (np.array([1000.25, 3000001.25]), np.array([2.0, 2.0]), 1000000), ["eager", "eager+long"],
          0, 0, 1, n_long=1, len_out=1997998),
        C("trim-exact-hit", _trim_curve(st0=1000.0), ["lazy"], 0, 0, 2),
        C("trim-in-segment-0", _trim_curve(n_in=1100), ["lazy"], 0, 0, 2),
        C("trim-in-last-segment", _trim_curve(n_in=512600), ["lazy"], 0, 0, 2),
        C("no-trim", _trim_curve(n_in=600000), ["lazy"], 0, 0, 2),
        C("serial-with-long-trim-sparse", _TRIM_SPARSE, ["serial"], 1, 0, 1, n_long=1, kwargs=dict(force_host_chain=1), len_out=1997998),
        C("serial-with-long-ramp", _SPARSE_RAMP, ["serial"], 1, 0, 1, n_long=2, kwargs=dict(force_host_chain=1)),
        C("ck-overflow-dense", lazy_plain, ["eager"], 0, 0, 0, kwargs=dict(eager=True, max_out=HALF)),
        C("ck-overflow-sparse", _SPARSE_RAMP, ["eager", "eager+long"], 0, 0, 0, n_long=1, kwargs=dict(eager=True, max_out=HALF)),
    ]


CASES = {c.name: c for c in _cases()}
# what each case is about; the CPU test holds every case clear of the others
TIE_CASES = {"lazy-length-ties", "lazy-length-ties-odd", "eager-length-ties", "mixed-long-length-ties", "sparse-length-tie", "cap-ambiguous-and-ties"}
CAP_CASES = {"cap-ambiguous-lazy", "cap-ambiguous-and-ties", "sparse-length-tie", "serial-with-long-trim-sparse", "range-behind-trim", "range-behind-trim-1e-4", "range-in-front",
             "trim-tie-sparse"}
RANGE_CASES = {"range-behind-trim", "range-behind-trim-1e-4", "range-in-front"}
TRIM_TIE_CASES = {"trim-tie-dense", "trim-tie-dense-eager", "trim-tie-sparse", "trim-tie-sparse-plain-cap", "trim-in-segment-0",
                  "trim-in-last-segment"}
