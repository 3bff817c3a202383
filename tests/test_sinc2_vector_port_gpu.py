"""The streaming kernel's per-pass vector bookkeeping (csrc/sinc2.hip, r10: the tile anchor's scalar case with the straddling
pass behind a branch, stores off a scalar base with a 32-bit byte offset, `c - ws` carried by the pass, the rows' block flags in
one test, the conversion verdict's ballots) against oracle_c (speed_to_pos + sinc) at the oracle's own positions.

Material: the 41-tile files of tests/test_sinc2_bookkeeping_gpu.py, computed once there and shared -- constant 0.994 (`a_slow`:
the order-5 loop of k_sinc_pipe<1, 2>), constant 1.006 (`a_fast`: the fc = 1 kernel <1, 1>) and the ramps `c` (all three
loops, regime changes inside streams).  All are free of window-centre ties (NOTES r09: the nearest position is 4.2e-6 from a
half-integer in c, 1e-3 in a), so their tile lists are empty and every pass that straddles a tile border -- one in eight -- is
placed by the hot loops.  A file this short runs as streams of three tiles (15-17 is one of them).

Bound: 1e-5 of the oracle's peak, everywhere.

Verdict cases.  A defect sits in the input of output tile 17, at least 520 samples behind the tile's first window centre and
ending 170 in front of the next tile's: the conversion runs 161 .. 473 samples ahead of the pass it leaves the loop with and a
chunk is 128 samples, so that pass (and the cold path's, whose ring starts 39 samples in front of its first centre) lies in
tile 17 whatever the chunk grid of the stream's ring; the ring restarted for tile 18 starts behind the defect.  The stretches
are 300 samples: any chunk grid has a whole chunk inside them."""
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
GUARD = 256
BAD_TILE = 17
MATERIAL = ("a_slow", "a_fast", "c")
DEFECTS = ("nan", "spike", "quiet", "zeros")


def _redo_list(plan, cap=64):
    """(length, sorted tiles) of the list the last fused launch on this plan left"""
    from pyaudiorestoration_amd import _dev, _lib
    buf = (ctypes.c_int * cap)()
    cnt = ctypes.c_int(-1)
    _lib.check(_lib.lib().par_fused_redo_list(0, _dev.ptr(plan.aux), plan.max_out, plan.m, buf, cap, ctypes.byref(cnt), _dev.stream_ptr(0)))
    return cnt.value, sorted(buf[i] for i in range(min(cnt.value, cap)))


def _rel(got, want, where=None, peak=None):
    """max |got - want| over the oracle's peak (the whole file's, NaNs aside, unless one is given)"""
    if peak is None:
        peak = float(np.nanmax(np.abs(want)))
    d = np.abs(got.astype(np.float64) - want)
    if where is not None:
        d = d[where]
    return float(np.max(d)) / peak


def _near_border(n):
    j = np.arange(n) % TILE
    return (j < 130) | (j >= TILE - 130)


@functools.lru_cache(maxsize=None)
def verdict_case(name, defect):
    """(signal, oracle output) of `name` with one defect in the input of output tile 17; read-only"""
    from oracle import oracle_c as C
    x, len_in, pos = B.case(name)[3:6]
    x = np.array(x)
    start = int(np.ceil(pos[BAD_TILE * TILE]))          # the tile's first window centre (speed ~ 1: a tile is ~1018 .. 1030 input samples)
    assert pos[(BAD_TILE + 1) * TILE] - start > 1000
    if defect == "nan":
        x[start + 700] = np.nan
    elif defect == "spike":
        x[start + 700:start + 764] = np.float32(40.0)
    elif defect == "quiet":                              # below 2^-13 = 1.22e-4 and nowhere zero
        q = x[start + 520:start + 820] * np.float32(2.0e-5)
        x[start + 520:start + 820] = np.where(q == 0.0, np.float32(1.0e-6), q)
        assert 0.0 < np.min(np.abs(x[start + 520:start + 820])) and np.max(np.abs(x[start + 520:start + 820])) < 2.0 ** -13
    else:
        x[start + 520:start + 820] = 0.0
    want = C.sinc(pos, x[:len_in], NT, threads=4)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def _launch_mono(name, x, guard=0):
    """one mono launch of the case's plan on signal x into a sentinel-filled buffer: (whole buffer, list length, tiles)"""
    import torch as t
    from pyaudiorestoration_amd import resampling
    len_in = B.case(name)[4]
    plan = B._plan(name)
    buf = t.full((guard + plan.len_out + guard,), SENTINEL, dtype=t.float32, device="cuda")
    resampling.varispeed_fused_dev(plan, t.from_numpy(np.array(x)).cuda(), NT, buf[guard:], len_in=len_in)
    n, tiles = _redo_list(plan)
    return buf.cpu().numpy(), n, tiles


@pytest.mark.parametrize("name", MATERIAL)
def test_tile_borders(name):
    """every output of the mono kernels, the passes that straddle a tile border among them: placed by the hot loops (empty list)"""
    want = B.case(name)[6]
    got, redo = B.run_mono(name)
    assert len(got) == len(want) and not np.any(got == SENTINEL)
    err, err_border = _rel(got, want), _rel(got, want, _near_border(len(want)))
    print(f"{name}: list {redo}, err {err!r}, within 130 of a tile border {err_border!r}")
    assert redo == 0, (name, redo)
    assert err < TOL and err_border < TOL, (name, err, err_border)


@pytest.mark.parametrize("name", MATERIAL)
def test_stereo_and_one_channel_of_frames(name):
    """the same material as an interleaved stereo file (k_sinc_pipe<2, 0>: left = noise, right = the tone) and each channel alone
    into its column of a frame buffer (<2, 3>, out_stride 2: the other column keeps its sentinel)"""
    import torch as t
    from pyaudiorestoration_amd import resampling
    len_in = B.case(name, "noise")[4]
    x_l, want_l = B.case(name, "noise")[3], B.case(name, "noise")[6]
    x_r, want_r = B.case(name, "tone")[3], B.case(name, "tone")[6]
    assert B.case(name, "tone")[4] == len_in
    plan = B._plan(name)
    inter = t.from_numpy(np.stack((x_l, x_r), axis=1)).cuda().reshape(-1)
    out = t.full((plan.len_out, 2), SENTINEL, dtype=t.float32, device="cuda")
    resampling.varispeed_fused_stereo_dev(plan, inter[0:], inter[1:], NT, out.reshape(-1)[0:], out.reshape(-1)[1:], sig_stride=2,
                                          len_in=len_in, out_stride=2)
    redo, _ = _redo_list(plan)
    o = out.cpu().numpy()
    near = _near_border(len(want_l))
    for label, got, want in (("left", o[:, 0], want_l), ("right", o[:, 1], want_r)):
        err, err_border = _rel(got, want), _rel(got, want, near)
        print(f"{name} stereo {label}: list {redo}, err {err!r}, within 130 of a tile border {err_border!r}")
        assert not np.any(got == SENTINEL) and err < TOL, (name, label, err)
    assert redo == 0, (name, redo)
    for ch, want in ((0, want_l), (1, want_r)):
        frames = t.full((plan.len_out, 2), SENTINEL, dtype=t.float32, device="cuda")
        resampling.varispeed_fused_dev(plan, inter[ch:], NT, frames.reshape(-1)[ch:], sig_stride=2, len_in=len_in, out_stride=2)
        redo, _ = _redo_list(plan)
        f = frames.cpu().numpy()
        err, err_border = _rel(f[:, ch], want), _rel(f[:, ch], want, near)
        print(f"{name} channel {ch} of the frames: list {redo}, err {err!r}, within 130 of a tile border {err_border!r}")
        assert np.all(f[:, 1 - ch] == SENTINEL), (name, ch)
        assert not np.any(f[:, ch] == SENTINEL) and err < TOL, (name, ch, err)
        assert redo == 0, (name, ch, redo)


@pytest.mark.parametrize("name", MATERIAL)
def test_mono_stores_stay_inside_the_output(name):
    """a sentinel in a guard stretch in front of `out` and behind len_out survives; none is left inside"""
    x, want = B.case(name)[3], B.case(name)[6]
    buf, redo, _ = _launch_mono(name, x, GUARD)
    n = len(want)
    assert len(buf) == n + 2 * GUARD
    assert np.all(buf[:GUARD] == SENTINEL) and np.all(buf[GUARD + n:] == SENTINEL), name
    got = buf[GUARD:GUARD + n]
    assert not np.any(got == SENTINEL), name
    assert np.array_equal(got, B.run_mono(name)[0]), name          # (the guard moves the base by 1 KiB: the same outputs)
    assert redo == 0, (name, redo)


@pytest.mark.parametrize("name", MATERIAL)
def test_stereo_stores_stay_inside_the_output(name):
    import torch as t
    from pyaudiorestoration_amd import resampling
    len_in = B.case(name, "noise")[4]
    x_l, want_l = B.case(name, "noise")[3], B.case(name, "noise")[6]
    x_r, want_r = B.case(name, "tone")[3], B.case(name, "tone")[6]
    plan = B._plan(name)
    n = plan.len_out
    inter = t.from_numpy(np.stack((x_l, x_r), axis=1)).cuda().reshape(-1)
    buf = t.full((GUARD + n + GUARD, 2), SENTINEL, dtype=t.float32, device="cuda")
    flat = buf[GUARD:].reshape(-1)
    resampling.varispeed_fused_stereo_dev(plan, inter[0:], inter[1:], NT, flat[0:], flat[1:], sig_stride=2, len_in=len_in, out_stride=2)
    o = buf.cpu().numpy()
    assert np.all(o[:GUARD] == SENTINEL) and np.all(o[GUARD + n:] == SENTINEL), name
    got = o[GUARD:GUARD + n]
    assert not np.any(got == SENTINEL), name
    assert _rel(got[:, 0], want_l) < TOL and _rel(got[:, 1], want_r) < TOL, name


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("name", ["a_fast", "a_slow"])
def test_conversion_verdicts(name, defect):
    """one NaN, 64 samples at 40.0, a chunk below 2^-13 that is not zero: tile 17 and no other goes to the list; a chunk of exact
    zeros: none does.  Finite outputs outside the listed tile stay within the bound (and the block kernel's inside it)."""
    x, want = verdict_case(name, defect)
    buf, redo, tiles = _launch_mono(name, x)
    tile = np.arange(len(want)) // TILE
    print(f"{name} {defect}: list {tiles}")
    assert (redo, tiles) == ((0, []) if defect == "zeros" else (1, [BAD_TILE])), (name, defect, redo, tiles)
    assert len(buf) == len(want) and not np.any(buf == SENTINEL)
    outside = tile != BAD_TILE
    assert np.isfinite(want[outside]).all() and np.isfinite(buf[outside]).all(), (name, defect)
    assert np.isnan(want).any() == (defect == "nan")                # (the case is what it says)
    # (outside the tile the outputs are the undisturbed file's: held to ITS peak, not to the 40.0 stretch's 45)
    err = _rel(buf, want, outside, float(np.max(np.abs(B.case(name)[6]))))
    inside = ~outside & np.isfinite(want) & np.isfinite(buf)
    err_in = _rel(buf, want, inside)
    print(f"{name} {defect}: err outside tile {BAD_TILE} {err!r}, finite outputs inside {err_in!r} ({int(inside.sum())} of {TILE})")
    assert err < TOL and err_in < TOL, (name, defect, err, err_in)


def test_three_files_in_one_launch():
    """0.994, the ramps and 1.006 with the 40.0 stretch in one par_varispeed_fused_batch_f32 launch (k_sinc_pipe_n): each file's
    output is its own launch's, bit for bit"""
    import torch as t
    from pyaudiorestoration_amd import resampling
    files = (("a_slow", None), ("c", None), ("a_fast", "spike"))
    plans, items, alone = [], [], []
    for nm, defect in files:
        st, sp, n, x, len_in = B.case(nm)[:5]
        if defect is not None:
            x = verdict_case(nm, defect)[0]
        alone.append(_launch_mono(nm, x)[0])
        plans.append(B._plan(nm))
        items.append(resampling.WorkItem(t.from_numpy(np.array(st)).cuda(), t.from_numpy(np.array(sp)).cuda(),
                                         t.from_numpy(np.array(x)).cuda(), 1, len_in))
    outs = resampling._resample_group(plans, items, NT, 0)
    for (nm, defect), o, own in zip(files, outs, alone):
        got = o.cpu().numpy()
        want = B.case(nm)[6] if defect is None else verdict_case(nm, defect)[1]
        assert _rel(got, want) < TOL, (nm, defect)
        assert np.array_equal(got, own), (nm, defect)
