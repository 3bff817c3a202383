"""CPU-only proof that the inputs of tests/fixed_rate_inputs.py do what tests/test_fixed_rate_kernels_gpu.py relies on: the sweep
shapes reach every allowed cell of the filter table with whole wings, an impulse train puts at most one impulse into any
output's window, and under fixed_rate_np.tolerance a shifted row, a dropped tap, a sample index off by one, swapped etas and a
tap taken past the count rule are each seen on the train outputs.  pytest -s prints the worst margins (NOTES.md, Fixed-ratio
resampler)."""
import numpy as np
import pytest

import fixed_rate_inputs as I
import fixed_rate_np as F
from test_fixed_rate_gpu import SHAPES

DIRECTIONS = [I.UP, I.DOWN]
CASES = [(z, a, b) for z in I.SWEPT_Z for a, b in DIRECTIONS]
IDS = [f"z{z}-{a}-{b}" for z, a, b in CASES]


def test_plan_is_the_oracle_bit_for_bit_on_the_existing_shapes():
    for a, b, n in SHAPES:
        x = np.random.default_rng(100 + n).uniform(-1, 1, n).astype(np.float32)
        y, K, B = F.oracle(x, a, b)
        pl = F.Plan(n, a, b)
        y2, K2, B2 = pl.evaluate(x)
        assert np.array_equal(y.view(np.int64), y2.view(np.int64)) and np.array_equal(K, K2) and np.array_equal(B.view(np.int64), B2.view(np.int64))
        for t in range(len(y)):                                   # the flat taps are taps() of every output
            jl, il, el, jr, ir, er, scale = F.taps(t, n, a, b)
            m = pl.o == t
            assert np.array_equal(pl.j[m], np.concatenate([jl, jr])) and np.array_equal(pl.i[m], np.concatenate([il, ir]))
            assert np.array_equal(pl.eta[m], np.concatenate([np.full(len(jl), el), np.full(len(jr), er)])) and scale == pl.scale
    for a, b, n, z in ((16, 1, 1200, 64), (1, 1.0 - 2.0 ** -52, 40, 8), (1, 1, 40, 5), (1, 16, 30, 8), (1023, 1024, 200, 1)):
        x = np.random.default_rng(n).uniform(-1, 1, n)            # the other shapes of the kernel tests, small
        for got, want in zip(F.Plan(n, a, b, num_zeros=z).evaluate(x), F.oracle(x, a, b, num_zeros=z)):
            assert np.array_equal(got, want)
    t0, t1 = 300, 420                                             # a range, and another table
    x = np.random.default_rng(1).uniform(-1, 1, 700)
    for got, want in zip(F.Plan(700, 48000, 44100, t0, t1, num_zeros=5).evaluate(x), F.oracle(x, 48000, 44100, t0, t1, num_zeros=5)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("z,a,b", CASES, ids=IDS)
def test_no_allowed_cell_is_left_unreached(z, a, b):
    pl = I.plan(a, b, z)
    allowed, reached = I.allowed_cells(pl), I.reached_cells(pl)
    print(f"num_zeros {z}, {a} -> {b}: {len(allowed)} allowed (wing, table index) cells, {len(reached)} reached with whole wings")
    assert reached == allowed
    if z == 8:
        assert len(allowed) == (7172 if (a, b) == I.UP else 7174)
    # both wings meet the last tap present (off <= 1 at ratio >= 1) and absent, on whole-wing outputs
    for wing in (0, 1):
        cnt = pl.cnt[wing][pl.whole]
        assert cnt.min() == z - 1 and cnt.max() == z


@pytest.mark.parametrize("z,a,b", CASES, ids=IDS)
def test_a_window_holds_one_impulse_at_most(z, a, b):
    pl = I.plan(a, b, z)
    S = I.train_period(z)
    full = max(F.uncut_count(t, a, b, z) for t in range(len(pl.K)))
    assert S & (S - 1) == 0 and S >= full >= pl.K.max() and S == {5: 16, 8: 16, 15: 32, 16: 32}[z]
    assert I.single_impulse(pl, S)
    Y, B = I.train_outputs(pl, S)
    for p in (0, 1, S - 1):                                        # the scattered form is the oracle on the train
        y, K, Bp = pl.evaluate(I.train(pl.n, S, p))
        assert np.array_equal(y, Y[p]) and np.array_equal(Bp, B[p]) and np.array_equal(K, pl.K)
    assert np.all(pl.w != 0) and np.count_nonzero(Y) == len(pl.w)  # every tap of every output stands alone once, none is a 0


@pytest.mark.parametrize("z,a,b", CASES, ids=IDS)
def test_wrong_kernels_are_seen_on_the_trains(z, a, b):
    pl = I.plan(a, b, z)
    S = I.train_period(z)
    allowed = I.allowed_cells(pl)
    rows = set(zip(pl.wing.tolist(), pl.off[pl.wing, pl.o].tolist()))

    shift = I.shift_margins(pl)                                    # every row, in either wing that reaches it
    assert set(shift) == rows and {r for _, r in rows} >= set(range(pl.step + 1))
    assert min(shift.values()) >= 1000

    drop = I.drop_margins(pl)                                      # every cell, at every output that reads it
    assert set(drop) == allowed and min(drop.values()) >= 100

    swap = I.eta_swap_margins(pl, 0.0)                             # every phase pair whose etas differ at all
    differ = pl.eta_out[0] != pl.eta_out[1]
    assert set(swap) == set(zip(pl.off[0][differ].tolist(), pl.off[1][differ].tolist()))
    if (a, b) == I.DOWN:
        assert len(swap) >= 1000 and min(swap.values()) >= 2       # 2: the wrong kernel's own rounding cannot hide it
    else:
        assert not differ.any()                                    # 1023 -> 1024: the etas are equal bit for bit, 0 or 0.5

    extra = I.extra_tap(pl, S)                                     # every row whose next entry is still in the table
    assert set(extra) == I.extra_rows(pl) and len(extra) >= 2 * (pl.step - 2)
    assert min(extra.values()) > 0.0
    print(f"num_zeros {z}, {a} -> {b}, tolerances: one-row shift >= {min(shift.values()):.0f} ({len(shift)} rows), dropped tap >= "
          f"{min(drop.values()):.0f} ({len(drop)} cells), swapped eta >= {min(swap.values()) if swap else float('nan'):.0f} ({len(swap)} pairs), "
          f"extra tap weight >= {min(extra.values()):.2e} where 0 is demanded ({len(extra)} rows)")


@pytest.mark.parametrize("z,a,b", [(8, *I.UP), (8, *I.DOWN), (16, *I.UP), (16, *I.DOWN)], ids=["z8-up", "z8-down", "z16-up", "z16-down"])
def test_nan_map_holds_both_wings_and_ends_where_the_count_rule_ends(z, a, b):
    pl = I.plan(a, b, z)
    q = I.NAN_Q
    hit, left, right = I.nan_map(pl, q)
    assert left.any() and right.any() and not (left & right).any()
    assert np.all(pl.whole[hit])                                   # q is far from the ends: the table alone limits these wings
    assert 2 * z - 2 <= hit.sum() <= 2 * z
    out_l, out_r = I.just_outside(pl, q)
    assert len(out_l) >= 1 and len(out_r) >= 1 and not hit[out_l].any() and not hit[out_r].any()
    if (z, a, b) == (8, *I.UP):                                    # distance exactly 7 to the left, 8 to the right, off >= 2
        assert np.all(pl.n0[out_l] - 7 == q) and np.all(pl.n0[out_r] + 8 == q)
        assert np.all(pl.off[0][out_l] >= 2) and np.all(pl.off[1][out_r] >= 2)
    # by hand from taps(): the same set
    want = [t for t in range(len(pl.K)) if q in F.taps(t, pl.n, a, b, z)[1] or q in F.taps(t, pl.n, a, b, z)[4]]
    assert np.array_equal(np.nonzero(hit)[0], want)
