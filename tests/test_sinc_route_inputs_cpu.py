"""Preconditions of tests/sinc_route_inputs.py, proved with the C oracle alone (no GPU): every curve gives the number of outputs
recorded beside it, untrimmed, with every position inside the signal; the named edge cases sit where the routing rule changes."""
import numpy as np
import pytest

import sinc_route_inputs as I


@pytest.mark.parametrize("name", sorted(I.CURVES))
def test_curve_gives_the_recorded_number_of_outputs(name):
    from oracle import oracle_c as C
    c = I.CURVES[name]
    st, sp = I.speed_curve(name)
    pos, trimmed = C.speed_to_pos(st, sp, c.n_in)
    assert len(pos) == c.len_out and not trimmed
    assert pos[0] > 0.0 and pos[-1] < c.n_in - 1 and np.all(np.diff(pos) > 0.0)
    step = np.diff(pos)
    assert step.min() < 1.0 < step.max() or c.base != 1.0            # both tap regimes (fc = 1 and fc < 1) in the unit-speed files


def test_edge_cases_sit_on_the_routing_edges():
    C = I.CURVES
    assert C["edge"].len_out == I.EDGE and C["edge"].n_in >= I.EDGE
    assert C["below"].len_out == I.EDGE - 1 and C["below"].n_in >= I.EDGE
    assert C["short_in"].len_out >= I.EDGE and C["short_in"].n_in == I.EDGE - 1
    assert C["edge_in"].len_out >= I.EDGE and C["edge_in"].n_in == I.EDGE
    assert all(C[n].len_out >= I.EDGE and C[n].n_in >= I.EDGE for n in I.MONO_NINE) and len(set(I.MONO_NINE)) == 9
    assert any(C[n].len_out % 1024 for n in I.MONO_NINE) and any(C[n].len_out % 1024 == 0 for n in I.MONO_NINE)


def test_signals_are_seeded_and_differ_per_channel():
    a, b = I.signal("edge"), I.signal("edge")
    assert a.dtype == np.float32 and a.shape == (I.CURVES["edge"].n_in,) and np.array_equal(a, b)
    s = I.signal("f3", 2)
    assert s.shape == (I.CURVES["f3"].n_in, 2) and not np.array_equal(s[:, 0], s[:, 1])
    assert not np.array_equal(I.signal("f1")[:4000], I.signal("f2")[:4000])
