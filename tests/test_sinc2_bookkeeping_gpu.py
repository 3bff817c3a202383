"""The streaming kernel's wave-uniform bookkeeping (csrc/sinc2.hip, r09: the loop's exit margin, the carried chunk source and
ring slot, dma_bad named where the ring is restarted, the tile cache) against oracle_c (speed_to_pos + sinc) at the oracle's
own positions, on files of at most 41 500 outputs -- the shapes of sinc2_loop_order_cases.py, whose figures bound them.

Cases (a file this short runs as streams of three tiles; the first, the last two full and the partial tile are end tiles):
    a  constant 0.994 (order-5 loop) and 1.006 (fc = 1 kernel); the input ends exactly where the last window needs it (one
       sample behind the last centre's 32nd tap), and 300 samples earlier.  On a file of 41 tiles the streams stop two tiles
       and more in front of the file's end, further than a ring reaches ahead: `a_cut` (added here) ends the input 2 600 samples
       early, INSIDE the streamed tiles, so that the last streams do meet chunks behind the file's end -- their passes leave
       the loop on the dma_bad margin, the chunk is fetched from the fallback source, the tiles go to the list.
    b  1 + 0.01 sin, period 25 tiles (every block a plain record, the list empty: `mixed25`); one NaN, and separately 64 samples
       at 40.0, in tile 17: the pass leaves the loop, the tile is pushed, the ring restarted behind it.
    c  1.006 -> 0.994 -> 0.9886 -> 1.006, plateaus ten tiles apart joined by ramps gentle enough for plain block records (at most
       2.2e-6 per sample; a step would flag its blocks cubic and hand their tiles to the block kernel): the fc = 1, order-5 and
       order-6 loops and the changes between them inside streams, with the records' guess moving.
    d  five full tiles and a partial one at 0.994: the smallest launch with end tiles (two streamed tiles).
    e  a and c as an interleaved stereo file (k_sinc_pipe<2, 0>), as one channel of it (<2, 3>), and as three files in one
       par_varispeed_fused_batch_f32 launch (bit-identical to their own launches).
Bounds: the contract's 1e-5 of the oracle's peak, and for the mono kernels 1.25 x what tests/test_sinc2_loop_orders_gpu.py holds
for the same material (its PARENT figures; for c, which crosses all three regimes, the largest of them).  The stereo and
one-channel forms: 1e-5, the bound of the streaming tests of those forms (tests/test_hip_parity.py)."""
import ctypes
import functools

import numpy as np
import pytest

import sinc2_loop_order_cases as K

pytestmark = pytest.mark.gpu

TOL = 1e-5
NT = 32
TILE = 1024
# tests/test_sinc2_loop_orders_gpu.py PARENT, per material (curve, signal)
HELD = {("fast", "noise"): 1.528e-06, ("fast", "tone"): 1.275e-06, ("slow", "noise"): 1.628e-06, ("slow", "tone"): 1.834e-06,
        ("order6", "noise"): 1.257e-06, ("order6", "tone"): 4.102e-06, ("mixed25", "noise"): 1.310e-06,
        ("mixed25", "tone"): 2.980e-06, ("list25", "noise"): 3.457e-07, ("list25", "tone"): 4.343e-07}
SPEED = {"fast": 1.006, "slow": 0.994}
BAD_TILE = 17


def _bound(material, sig):
    if material == "ramps":
        return 1.25 * max(HELD[(m, sig)] for m in ("fast", "slow", "order6", "mixed25"))
    return 1.25 * HELD[(material, sig)]


def _signal(sig, n):
    if sig == "noise":
        x = np.random.default_rng(9).standard_normal(n)
        return (0.5 * x / np.max(np.abs(x))).astype(np.float32)
    return np.cos(0.98 * np.pi * np.arange(n) + 0.3).astype(np.float32)


def _ramps(st):
    """1.006 -> 0.994 -> 0.9886 -> 1.006 over output tiles 10, 20, 30 (input sample ~ output sample), linear ramps of 6, 6 and
    9 tiles: 2.0e-6, 0.9e-6 and 1.9e-6 per sample"""
    knots = np.array([0, 7, 13, 17, 23, 25.5, 34.5, 42]) * TILE
    return np.interp(st, knots, [1.006, 1.006, 0.994, 0.994, 0.9886, 0.9886, 1.006, 1.006])


@functools.lru_cache(maxsize=None)
def case(name, sig="noise"):
    """(sampletimes, speeds, n, signal, len_in, oracle positions, oracle output, material); computed once, read-only"""
    from oracle import oracle_c as C
    out_target = 5 * TILE + 540 if name == "d" else K.OUT_TARGET
    if name in ("a_slow", "a_slow_300", "a_slow_cut", "d"):
        material, speed = "slow", SPEED["slow"]
    elif name in ("a_fast", "a_fast_300", "a_fast_cut"):
        material, speed = "fast", SPEED["fast"]
    elif name == "c":
        material, speed = "ramps", 1.0
    else:
        material, speed = ("mixed25" if name == "b_nan" else "list25"), 1.0
    n = int(round(out_target / speed))
    st = np.linspace(0, n, n // 256)
    if name == "c":
        sp = _ramps(st)
    elif name.startswith("b_"):
        sp = 1.0 + 0.01 * np.sin(2.0 * np.pi * st / (25.0 * TILE))
    else:
        sp = np.full(len(st), speed)
    pos, _ = C.speed_to_pos(st, sp, n)
    last = int(np.rint(pos[-1])) + NT + 1         # one sample behind the last window
    x = _signal(sig, max(n, last) + 64)
    len_in = n
    if name.startswith("a_"):
        len_in = last - (300 if name.endswith("_300") else 2600 if name.endswith("_cut") else 0)
    at = BAD_TILE * TILE + 500                    # (speed ~ 1: input sample ~ output sample, +- 40: inside tile 17 with its window)
    if name == "b_nan":
        x[at] = np.nan
    if name == "b_spike":
        x[at:at + 64] = np.float32(40.0)
    want = C.sinc(pos, x[:len_in], NT, threads=4)
    for a in (st, sp, x, pos, want):
        a.setflags(write=False)
    return st, sp, n, x, len_in, pos, want, material


def _plan(name, sig="noise"):
    import torch as t
    from pyaudiorestoration_amd import resampling
    st, sp, n = case(name, sig)[:3]
    plan = resampling.speed_plan_dev(t.from_numpy(np.array(st)).cuda(), t.from_numpy(np.array(sp)).cuda(), n, fused=True)
    assert plan.fused_ok
    return plan


def _redo(plan):
    from pyaudiorestoration_amd import _dev, _lib
    redo = ctypes.c_int(-1)
    _lib.check(_lib.lib().par_fused_redo_tiles(0, _dev.ptr(plan.aux), plan.max_out, plan.m, ctypes.byref(redo), _dev.stream_ptr(0)))
    return redo.value


@functools.lru_cache(maxsize=None)
def run_mono(name, sig="noise"):
    """(output, tiles in the list) of one mono case on the GPU (k_sinc_pipe<1, 2> + <1, 1>)"""
    import torch as t
    from pyaudiorestoration_amd import resampling
    x, len_in = case(name, sig)[3:5]
    plan = _plan(name, sig)
    out = t.full((plan.len_out,), 7.0, dtype=t.float32, device="cuda")
    resampling.varispeed_fused_dev(plan, t.from_numpy(np.array(x)).cuda(), NT, out, len_in=len_in)
    redo = _redo(plan)
    got = out.cpu().numpy()
    got.setflags(write=False)
    return got, redo


def _err(got, want, where=None):
    d = np.abs(got.astype(np.float64) - want)
    if where is not None:
        d, want = d[where], want[where]
    return float(np.max(d)) / float(np.max(np.abs(want)))


def _check(label, got, want, bound, where=None):
    assert len(got) == len(want), (label, len(got), len(want))
    assert not np.any(got[where if where is not None else slice(None)] == 7.0), label
    err = _err(got, want, where)
    print(f"{label}: err {err!r} bound {bound!r}")
    assert err < TOL and err <= bound, (label, err, bound)


@pytest.mark.parametrize("name", ["a_slow", "a_slow_300", "a_fast", "a_fast_300", "c", "d"])
def test_mono_against_the_oracle(name):
    want, material = case(name)[6:8]
    got, redo = run_mono(name)
    print(f"{name}: list {redo}")
    _check(name, got, want, _bound(material, "noise"))
    if name != "c":
        assert redo == 0, (name, redo)           # constant curves: every streamed tile ran in its loop
    else:
        assert 0 <= redo < 37, (name, redo)


@pytest.mark.parametrize("name", ["a_slow_cut", "a_fast_cut"])
def test_input_ends_inside_the_streamed_tiles(name):
    want, material = case(name)[6:8]
    got, redo = run_mono(name)
    print(f"{name}: list {redo}")
    _check(name, got, want, _bound(material, "noise"))
    assert 1 <= redo < 37, (name, redo)          # the streams that met the file's end handed their tiles over


def test_nan_in_one_tile():
    want = case("b_nan")[6]
    got, redo = run_mono("b_nan")
    print(f"b_nan: list {redo}, NaN outputs {int(np.isnan(got).sum())} (oracle {int(np.isnan(want).sum())})")
    assert redo >= 1, redo
    tile = np.arange(len(got)) // TILE
    assert not np.isnan(got[tile != BAD_TILE]).any()
    assert np.isnan(want).any() and not np.isnan(want[tile != BAD_TILE]).any()      # (the case is what it says)
    _check("b_nan", got, want, _bound("mixed25", "noise"), tile != BAD_TILE)
    both = (tile == BAD_TILE) & np.isfinite(want) & np.isfinite(got)
    assert both.any()
    _check("b_nan, tile 17", got, want, _bound("mixed25", "noise"), both)


def test_spike_in_one_tile():
    want = case("b_spike")[6]
    got, redo = run_mono("b_spike")
    print(f"b_spike: list {redo}")
    assert redo >= 1, redo
    _check("b_spike", got, want, _bound("list25", "noise"))


@pytest.mark.parametrize("name", ["a_slow", "a_slow_300", "a_fast", "a_fast_300", "c"])
def test_stereo_and_one_channel(name):
    """left = the case's noise, right = the tone on the same curve: k_sinc_pipe<2, 0>, then each channel alone through <2, 3>"""
    import torch as t
    from pyaudiorestoration_amd import resampling
    len_in, _, want_l = case(name, "noise")[4:7]
    x_l, x_r, want_r = case(name, "noise")[3], case(name, "tone")[3], case(name, "tone")[6]
    assert case(name, "tone")[4] == len_in
    plan = _plan(name)
    inter = t.from_numpy(np.stack((x_l, x_r), axis=1)).cuda().reshape(-1)
    out = t.full((plan.len_out, 2), 7.0, dtype=t.float32, device="cuda")
    resampling.varispeed_fused_stereo_dev(plan, inter[0:], inter[1:], NT, out.reshape(-1)[0:], out.reshape(-1)[1:], sig_stride=2,
                                          len_in=len_in, out_stride=2)
    redo = _redo(plan)
    o = out.cpu().numpy()
    print(f"{name} stereo: list {redo}")
    _check(f"{name} stereo left", o[:, 0], want_l, TOL)
    _check(f"{name} stereo right", o[:, 1], want_r, TOL)
    assert redo == 0 if name != "c" else redo < 37, (name, redo)
    for ch, want in ((0, want_l), (1, want_r)):
        one = t.full((plan.len_out,), 7.0, dtype=t.float32, device="cuda")
        resampling.varispeed_fused_dev(plan, inter[ch:], NT, one, sig_stride=2, len_in=len_in)
        redo = _redo(plan)
        _check(f"{name} channel {ch} of the frames", one.cpu().numpy(), want, TOL)
        assert redo == 0 if name != "c" else redo < 37, (name, ch, redo)


def test_three_files_in_one_launch():
    """a (0.994, input ending at the last window), c and a (1.006, 300 samples short) in one par_varispeed_fused_batch_f32
    launch: each file's output is its own launch's, bit for bit"""
    import torch as t
    from pyaudiorestoration_amd import resampling
    names = ("a_slow", "c", "a_fast_300")
    plans, items = [], []
    for nm in names:
        st, sp, n, x, len_in = case(nm)[:5]
        plans.append(_plan(nm))
        items.append(resampling.WorkItem(t.from_numpy(np.array(st)).cuda(), t.from_numpy(np.array(sp)).cuda(),
                                         t.from_numpy(np.array(x)).cuda(), 1, len_in))
    outs = resampling._resample_group(plans, items, NT, 0)
    for nm, o in zip(names, outs):
        want, material = case(nm)[6:8]
        got = o.cpu().numpy()
        _check(f"{nm} in the batch", got, want, _bound(material, "noise"))
        assert np.array_equal(got, run_mono(nm)[0]), nm
