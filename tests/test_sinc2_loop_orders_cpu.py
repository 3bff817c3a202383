"""The oracle side of test_sinc2_loop_orders_gpu.py, without a GPU: every curve of sinc2_loop_order_cases.py gives 40 full
tiles and a partial one, finite positions and a finite oracle output of that length, with the tap regime it is named for."""
import numpy as np
import pytest

import sinc2_loop_order_cases as K


@pytest.mark.parametrize("curve", K.CURVES)
def test_oracle_is_finite_and_has_the_expected_length(curve):
    for sig in K.SIGNALS:
        st, sp, n, x, pos, want = K.case(curve, sig)
        assert len(pos) == len(want)
        assert 40 * K.TILE < len(want) < 41 * K.TILE, len(want)          # 40 full tiles + a partial one
        assert abs(len(want) - K.OUT_TARGET) <= 100, len(want)             # (a sine that ends inside a period shifts the mean speed)
        assert np.all(np.isfinite(pos)) and np.all(np.isfinite(want))
        assert np.all(np.diff(pos) > 0) and pos[0] >= 0 and pos[-1] < n
        assert len(x) == n and np.all(np.isfinite(x))
        peak = float(np.max(np.abs(want)))
        if curve in ("list", "list25"):
            assert peak > 32.0                                           # the spike reaches the output: beyond the images' range
        else:
            assert 0.3 < peak < 1.5, peak


def test_curves_sit_in_their_regimes():
    """period = 1 / speed (checked on the oracle's own positions); fc < 1 where it exceeds 1, and 1 - fc = 1 - 1 / period"""
    for name, s in K.CONSTANT.items():
        pos = K.case(name, "tone")[4]
        assert np.allclose(np.diff(pos), 1.0 / s, rtol=0, atol=1e-9), name
    g = lambda s: 1.0 - s                        # 1 - fc of a speed < 1
    assert K.CONSTANT["fast6"] > 1.0 and K.CONSTANT["fast115"] > 1.0                 # fc = 1
    assert 0.0 < g(K.CONSTANT["slow6"]) <= 0.0105                                    # order 5
    assert 0.0105 < g(K.CONSTANT["order6"]) <= 0.0125                                # order 6
    for name, flips_want in (("mixed", (5, 8)), ("mixed25", (2, 4))):
        st, sp, n = K.curve(name)
        assert sp.min() < 1.0 < sp.max() and g(sp.min()) <= 0.0105
        # regime changes inside the file, whole streams (three tiles) on either side
        flips = np.count_nonzero(np.diff(np.signbit(sp - 1.0)))
        assert flips_want[0] <= flips <= flips_want[1], (name, flips)
        # the plan's records are plain quadratics up to a speed step of 2.7e-6 x speed per sample (seg_fast_record): `mixed25`
        # stays inside it everywhere, the issue's 12-tile period does not (its flanks are the block kernel's)
        step = np.max(np.abs(np.diff(sp)) / (np.diff(st) - 1.0))
        assert (step <= 0.95 * 2.7e-6 * sp.min()) == (name == "mixed25"), (name, step)


@pytest.mark.parametrize("curve", ["list", "list25"])
def test_spike_lies_inside_one_tile(curve):
    st, sp, n, x, pos, want = K.case(curve, "noise")
    hit = np.nonzero(np.abs(x) >= 32.0)[0]
    assert len(hit) == K.SPIKE_LEN
    outs = np.nonzero((pos > hit[0] - 1) & (pos < hit[-1] + 1))[0]       # outputs centred on the spike
    assert len(outs) and outs[0] // K.TILE == outs[-1] // K.TILE
    assert 1 <= outs[0] // K.TILE < 38                                   # a streamed tile, not an end tile
