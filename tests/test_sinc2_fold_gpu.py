"""The folded third K slice of the streaming kernel's banks (csrc/sinc2.hip, r11: the overhang taps 33 - i .. 31 of sub-position
i >= 2 -- slice 2 of the dominant filter pairs -- enter through ONE MFMA with the constant fragment V and the mixed signal
fragment xv) against oracle_c (speed_to_pos + sinc) at the oracle's own positions.

Material: the 41-tile curves of tests/test_sinc2_bookkeeping_gpu.py -- constant 0.994 (`a_slow`: the order-5 loop of
k_sinc_pipe<1, 2>), constant 1.006 (`a_fast`: the fc = 1 kernel <1, 1>) and the ramps `c` (all three loops of <1, 2>, the
order-6 loop with its three full slices among them, and the changes between them, where the wave swaps the folded fragments
for the slice-2 fragments and back).  They are free of window-centre ties, so the tile list stays empty: every output below is
a streaming kernel's.  Signals, so that a misplaced element of V or lane of xv shows:
    imp0    unit impulses 67 samples apart (one per 64-tap window, every residue mod 8) over EXACT zeros: an output sees an impulse
            at one tap and nothing else, so a missing overhang tap is missing from it -- tap 31 weighs 2.4e-5 of the peak at a
            shift of 1/2, tap 26 1e-3
    imp3    the same impulses over 1e-3 noise
    steps   1 + m 2^-13, m uniform in -2048 .. 2047: the images' lo parts carry the whole difference between samples
Coverage of the impulses is asserted from the oracle's positions: within every aligned three tiles (a stream of these files),
for every residue mod 8 of the window centre and every tap 26 .. 31 some output has an impulse at that tap.  A stream's
sub-position (c - ws) & 7 is the centre's residue mod 8 shifted by the stream's (even) anchor, so every sub-position 2 .. 7 meets
every one of its overhang taps in every stream; errors are printed per residue class.

Bounds: 1e-5 of the oracle's peak (the contract), and <= 1.25 x the error of the parent build (three full slices, 13 / 28
MFMAs) on the same case, measured once on an MI355X through PAR_HIP_LIB and recorded in PARENT."""
import ctypes
import functools

import numpy as np
import pytest

import test_sinc2_bookkeeping_gpu as B

pytestmark = pytest.mark.gpu

TOL = 1e-5
NT = B.NT
TILE = B.TILE
SENTINEL = 7.0
BAD_TILE = 17
MATERIAL = ("a_slow", "a_fast", "c")
SIGNALS = ("imp0", "imp3", "steps")
IMP_FIRST, IMP_STEP = 100, 67
# max |got - oracle| / max |oracle| of the parent build on these very cases (MI355X)
PARENT = {
    ("a_slow", "imp0"): 6.371e-07, ("a_slow", "imp3"): 6.521e-07, ("a_slow", "steps"): 2.372e-06,
    ("a_fast", "imp0"): 6.258e-07, ("a_fast", "imp3"): 6.482e-07, ("a_fast", "steps"): 2.453e-06,
    ("c", "imp0"): 6.259e-07, ("c", "imp3"): 6.482e-07, ("c", "steps"): 2.465e-06,
    ("a_slow", "stereo", 0): 6.521e-07, ("a_slow", "stereo", 1): 2.372e-06,
    ("a_slow", "frames", 0): 6.521e-07, ("a_slow", "frames", 1): 2.372e-06,
    ("a_fast", "stereo", 0): 6.482e-07, ("a_fast", "stereo", 1): 2.453e-06,
    ("a_fast", "frames", 0): 6.482e-07, ("a_fast", "frames", 1): 2.453e-06,
    ("c", "stereo", 0): 6.482e-07, ("c", "stereo", 1): 2.465e-06,
    ("c", "frames", 0): 6.482e-07, ("c", "frames", 1): 2.465e-06,
    ("a_slow", "nan"): 6.521e-07, ("a_fast", "nan"): 6.482e-07,
}


def _signal(sig, n):
    rng = np.random.default_rng(11)
    if sig == "steps":
        return (1.0 + rng.integers(-2048, 2048, n) * 2.0 ** -13).astype(np.float32)
    x = np.zeros(n, dtype=np.float32) if sig == "imp0" else (1e-3 * rng.standard_normal(n)).astype(np.float32)
    x[IMP_FIRST::IMP_STEP] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def case(name, sig):
    """(signal, len_in, oracle positions, oracle output); computed once, read-only"""
    from oracle import oracle_c as C
    x0, len_in, pos = B.case(name)[3:6]
    x = _signal(sig, len(x0))
    want = C.sinc(pos, x[:len_in], NT, threads=4)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, len_in, pos, want


def _redo_list(plan, cap=64):
    from pyaudiorestoration_amd import _dev, _lib
    buf = (ctypes.c_int * cap)()
    cnt = ctypes.c_int(-1)
    _lib.check(_lib.lib().par_fused_redo_list(0, _dev.ptr(plan.aux), plan.max_out, plan.m, buf, cap, ctypes.byref(cnt), _dev.stream_ptr(0)))
    return cnt.value, sorted(buf[i] for i in range(min(cnt.value, cap)))


@functools.lru_cache(maxsize=None)
def run_mono(name, sig):
    """(output, tiles in the list) of one mono launch (k_sinc_pipe<1, 2> + <1, 1>)"""
    import torch as t
    from pyaudiorestoration_amd import resampling
    x, len_in = case(name, sig)[:2]
    plan = B._plan(name)
    out = t.full((plan.len_out,), SENTINEL, dtype=t.float32, device="cuda")
    resampling.varispeed_fused_dev(plan, t.from_numpy(np.array(x)).cuda(), NT, out, len_in=len_in)
    redo = _redo_list(plan)[0]
    got = out.cpu().numpy()
    got.setflags(write=False)
    return got, redo


def _check(key, got, want, pos, where=None):
    """err of `got` against the oracle, printed overall and per residue mod 8 of the window centre, held to both bounds"""
    assert len(got) == len(want), (key, len(got), len(want))
    sel = np.ones(len(want), dtype=bool) if where is None else where
    assert not np.any(got[sel] == SENTINEL), key
    peak = float(np.max(np.abs(want[sel])))
    d = np.abs(got.astype(np.float64) - want) / peak
    res = np.rint(pos).astype(np.int64) & 7
    by = [float(np.max(d[sel & (res == r)])) for r in range(8)]
    err = float(np.max(d[sel]))
    print(f"FIG {key!r}: {err:.3e},   by residue " + " ".join(f"{e:.2e}" for e in by) + f"   parent {PARENT.get(key)}")
    assert err < TOL, (key, err)
    assert err <= 1.25 * PARENT[key], (key, err, PARENT[key])


def _impulse_coverage(pos, len_in):
    """every (centre residue mod 8, overhang tap 26 .. 31) pair is met within every aligned three tiles"""
    c = np.rint(pos).astype(np.int64)
    for t0 in range(0, len(pos) // TILE - 2, 3):
        cc = c[t0 * TILE:(t0 + 3) * TILE]
        have = set()
        for n in range(26, 32):
            p = cc + n
            hit = (p >= IMP_FIRST) & (p < len_in) & ((p - IMP_FIRST) % IMP_STEP == 0)
            have |= {(int(r), n) for r in np.unique(cc[hit] & 7)}
        assert len(have) == 8 * 6, (t0, sorted(set((r, n) for r in range(8) for n in range(26, 32)) - have))


@pytest.mark.parametrize("sig", SIGNALS)
@pytest.mark.parametrize("name", MATERIAL)
def test_mono(name, sig):
    """both mono kernels, every loop: the list stays empty, every output is written"""
    x, len_in, pos, want = case(name, sig)
    if sig != "steps":
        _impulse_coverage(pos, len_in)
    got, redo = run_mono(name, sig)
    assert redo == 0, (name, sig, redo)
    _check((name, sig), got, want, pos)


@pytest.mark.parametrize("name", MATERIAL)
def test_stereo_and_one_channel_of_frames(name):
    """an interleaved stereo file (k_sinc_pipe<2, 0>: left = imp3, right = steps) and each channel alone into its column of a
    frame buffer (<2, 3>: the other column keeps its sentinel)"""
    import torch as t
    from pyaudiorestoration_amd import resampling
    x_l, len_in, pos, want_l = case(name, "imp3")
    x_r, _, _, want_r = case(name, "steps")
    plan = B._plan(name)
    inter = t.from_numpy(np.stack((x_l, x_r), axis=1)).cuda().reshape(-1)
    out = t.full((plan.len_out, 2), SENTINEL, dtype=t.float32, device="cuda")
    resampling.varispeed_fused_stereo_dev(plan, inter[0:], inter[1:], NT, out.reshape(-1)[0:], out.reshape(-1)[1:], sig_stride=2,
                                          len_in=len_in, out_stride=2)
    assert _redo_list(plan)[0] == 0, name
    o = out.cpu().numpy()
    _check((name, "stereo", 0), o[:, 0], want_l, pos)
    _check((name, "stereo", 1), o[:, 1], want_r, pos)
    for ch, want in ((0, want_l), (1, want_r)):
        frames = t.full((plan.len_out, 2), SENTINEL, dtype=t.float32, device="cuda")
        resampling.varispeed_fused_dev(plan, inter[ch:], NT, frames.reshape(-1)[ch:], sig_stride=2, len_in=len_in, out_stride=2)
        assert _redo_list(plan)[0] == 0, (name, ch)
        f = frames.cpu().numpy()
        assert np.all(f[:, 1 - ch] == SENTINEL), (name, ch)
        _check((name, "frames", ch), f[:, ch], want, pos)


def test_three_files_in_one_launch():
    """0.994 with the impulses, the ramps with the steps and 1.006 with the impulses over noise in one
    par_varispeed_fused_batch_f32 launch (k_sinc_pipe_n): each file's output is its own launch's, bit for bit"""
    import torch as t
    from pyaudiorestoration_amd import resampling
    files = (("a_slow", "imp0"), ("c", "steps"), ("a_fast", "imp3"))
    plans, items = [], []
    for nm, sig in files:
        st, sp = B.case(nm)[:2]
        x, len_in = case(nm, sig)[:2]
        plans.append(B._plan(nm))
        items.append(resampling.WorkItem(t.from_numpy(np.array(st)).cuda(), t.from_numpy(np.array(sp)).cuda(),
                                         t.from_numpy(np.array(x)).cuda(), 1, len_in))
    outs = resampling._resample_group(plans, items, NT, 0)
    for (nm, sig), o in zip(files, outs):
        got = o.cpu().numpy()
        assert not np.any(got == SENTINEL), (nm, sig)
        assert np.array_equal(got, run_mono(nm, sig)[0]), (nm, sig)


@pytest.mark.parametrize("name", ["a_slow", "a_fast"])
def test_nan_in_an_overhang_stretch(name):
    """One NaN in the input of tile 17, at least 700 samples behind the tile's first window centre.  Every image sample lies at K
    entries 64 .. 71 of one block of its pass (the blocks are 8 centres apart, xv reads 8 samples), so the mixed fragment of
    some pass reads it from the hi image, the lanes g = 2 from the lo image: the conversion that wrote both sends tile 17, and
    no other, to the list; outputs of the other tiles are finite and within the bound."""
    import torch as t
    from oracle import oracle_c as C
    from pyaudiorestoration_amd import resampling
    x, len_in, pos, _ = case(name, "imp3")
    x = np.array(x)
    start = int(np.ceil(pos[BAD_TILE * TILE]))
    assert pos[(BAD_TILE + 1) * TILE] - start > 1000
    x[start + 700] = np.nan
    want = C.sinc(pos, x[:len_in], NT, threads=4)
    plan = B._plan(name)
    out = t.full((plan.len_out,), SENTINEL, dtype=t.float32, device="cuda")
    resampling.varispeed_fused_dev(plan, t.from_numpy(x).cuda(), NT, out, len_in=len_in)
    redo, tiles = _redo_list(plan)
    got = out.cpu().numpy()
    assert (redo, tiles) == (1, [BAD_TILE]), (name, redo, tiles)
    outside = np.arange(len(want)) // TILE != BAD_TILE
    assert np.isnan(want).any() and np.isfinite(want[outside]).all()
    assert np.isfinite(got[outside]).all(), name
    _check((name, "nan"), got, want, pos, outside)
