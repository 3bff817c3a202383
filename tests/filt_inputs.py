"""Cascades, signals and lengths of the K_sosfiltfilt pins (test_filt_cpu.py, test_filt_kernels_gpu.py).

The cascades are the narrow bands the wow and lag tools design (poles within 1e-4 of z = 1, where the 2x2 block matrices nearly
cancel), the wide ones the older tests use, and the shapes of a cascade that change a code path (one section with zero
coefficients, twelve sections).  The lengths are chosen by the EXTENDED length L = n + 2 padlen, which is what the kernels cut
into 256-sample blocks and 256-block super-blocks."""
import collections
import functools

import numpy as np
import scipy.signal

BLOCK = 256                      # kFiltBlock
SUPER = 256                      # kFiltSuper: blocks per super-block
FLOOR = 8 * 2.0 ** -53           # below this an error ratio compares rounding of the output itself
# The pin of both entry points (test_filt_kernels_gpu.py):  e_gpu <= R max(e_scipy, FLOOR), e = max |y - oracle| / max |oracle|.
# R = 3 x the worst ratio measured on the MI355X over every cascade, signal and length below, 4.97 (NOTES.md, "K_sosfiltfilt
# against a long-double oracle"; the factor 3 is how far the ratio moves with the seed); the issue that asked for the pin caps it at 64.
R = 15.0

Cascade = collections.namedtuple("Cascade", "name sos padlen narrow")


def padlen_of(sos):
    """scipy.signal.sosfiltfilt's default padlen"""
    ntaps = 2 * sos.shape[0] + 1
    ntaps -= min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum()))
    return 3 * ntaps


def _butter(order, lo, hi, fs, btype):
    nyq = 0.5 * fs
    wn = {"band": [lo / nyq, hi / nyq], "low": hi / nyq, "high": lo / nyq}[btype]
    return np.ascontiguousarray(scipy.signal.butter(order, wn, btype=btype, output="sos"), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def cascades():
    spec = [
        # name, order, low edge, high edge, fs, type, narrow
        ("band_300_3000_48k_o3", 3, 300.0, 3000.0, 48000.0, "band", False),
        ("low_2_44k_o3", 3, 0.0, 2.0, 44100.0, "low", True),
        ("band_1_2_44k_o3", 3, 1.0, 2.0, 44100.0, "band", True),
        ("band_20_40_48k_o3", 3, 20.0, 40.0, 48000.0, "band", True),
        ("high_5_48k_o5", 5, 5.0, 0.0, 48000.0, "high", True),
        ("band_50_60_48k_o5", 5, 50.0, 60.0, 48000.0, "band", True),
        ("golden_low_20_172", 3, 0.0, 20.0, 172.265625, "low", False),         # test_filters_golden's two
        ("golden_high_300_44k", 3, 300.0, 0.0, 44100.0, "high", False),
        ("band_9990_10010_48k_o5", 5, 9990.0, 10010.0, 48000.0, "band", True),  # narrow, but far from z = 1
        ("one_section_low", 1, 0.0, 2400.0, 48000.0, "low", False),            # b2 = a2 = 0: padlen 6, not 9
        ("twelve_sections", 12, 1200.0, 7200.0, 48000.0, "band", False),
    ]
    out = []
    for name, order, lo, hi, fs, btype, narrow in spec:
        sos = _butter(order, lo, hi, fs, btype)
        out.append(Cascade(name, sos, padlen_of(sos), narrow))
    assert out[-2].sos.shape[0] == 1 and out[-2].padlen == 6 and out[-1].sos.shape[0] == 12
    return tuple(out)


def cascade(name):
    return next(c for c in cascades() if c.name == name)


CASCADE_NAMES = tuple(c.name for c in cascades())
NARROW_NAMES = tuple(c.name for c in cascades() if c.narrow)


@functools.lru_cache(maxsize=None)
def narrow_trio():
    """three different narrow cascades of one shape (order-3 band-passes: three sections, padlen 21) for one batch"""
    trio = (cascade("band_1_2_44k_o3"), cascade("band_20_40_48k_o3"),
            Cascade("band_5_10_44k_o3", _butter(3, 5.0, 10.0, 44100.0, "band"), 21, True))
    assert {c.padlen for c in trio} == {21} and {c.sos.shape[0] for c in trio} == {3}
    return trio


def lengths(padlen):
    """[(label, n)]: the signal lengths whose extended length L = n + 2 padlen sits on the seams of the block structure"""
    out = [("one_block", padlen + 1)]
    for L in (BLOCK - 1, BLOCK, BLOCK + 1,                                   # first block seam
              BLOCK * SUPER - 1, BLOCK * SUPER, BLOCK * SUPER + 1,             # first super-block seam
              4 * BLOCK * SUPER, 4 * BLOCK * SUPER + 1):                       # nsup 4 -> 5 (where the single form once changed chains)
        out.append((f"L{L}", L - 2 * padlen))
    out.append(("n600001", 600001))                                            # several super-blocks
    return out


LENGTH_LABELS = tuple(label for label, _ in lengths(21))
SIGNAL_NAMES = ("noise_dc", "impulse_seam", "step", "ramp")


def seam_index(n, padlen):
    """the sample whose EXTENDED index is the first index of a block in the middle of the signal (n // 2 when there is one block)"""
    L = n + 2 * padlen
    k = (L // BLOCK) // 2
    i = k * BLOCK - padlen
    return i if k >= 1 and 0 < i < n else n // 2


def signal(name, n, padlen, seed=0):
    if name == "noise_dc":
        return np.random.default_rng(1000 + seed).standard_normal(n) + 0.5
    if name == "impulse_seam":
        x = np.zeros(n)
        x[seam_index(n, padlen)] = 1.0
        return x
    if name == "step":
        x = np.zeros(n)
        x[n // 3:] = 1.0
        return x
    if name == "ramp":                       # the odd extension continues a ramp: ext[i] = x[0] + (i - padlen) * slope up to rounding
        return -0.7 + np.arange(n) * (2.0 / n)
    raise KeyError(name)


def rel_err(y, ref):
    """max |y - ref| / max |ref|"""
    return float(np.max(np.abs(np.asarray(y) - ref)) / np.max(np.abs(ref)))
