"""The streaming kernel's mono hot loops (csrc/sinc2.hip: k_sinc_pipe<1, 2> and <1, 1>) against oracle_c (speed_to_pos + sinc)
on the smallest files that still enter each loop and leave it again -- sinc2_loop_order_cases.py has the shapes, the curves
and the signals.  What pins an iteration's order of stages: a loop that reads a bank row, an image fragment or a record a
stage too early or too late computes from the wrong pass, which no listing shows and every one of these files does.

Bounds: the contract's 1e-5 of the oracle's peak, and per case 1.25 x what the r06 loop order (the parent of the stage-ahead
order) measured on the same file -- headroom for a different FMA contraction, nothing more.  PARENT holds those figures.
Coverage: len_out is the oracle's; the output, prefilled with 7.0, is written everywhere; the tile list, read back after the
launch, is EMPTY on the constant curves and on `mixed25` -- every pass ran in the loop the curve is meant for, none through the
block kernel -- and fills on `list25`.  The 12-tile sine (`mixed`, `list`) cannot keep the list empty: its flanks are steeper than
the plan's plain block records go, and those tiles are the block kernel's by design (28 of the file's 41, the end tiles not
counted); there the list must hold some tiles but not all, and one more with the spike than without."""
import ctypes
import functools

import numpy as np
import pytest

import sinc2_loop_order_cases as K

pytestmark = pytest.mark.gpu

TOL = 1e-5
# max |got - oracle| / max |oracle| of the r06 loop order (PAR_S3_EARLY_LDS=0 of the commit that introduced the stage-ahead
# order), measured on an MI355X on these very files
PARENT = {
    ("fast6", "noise"): 1.528e-06, ("fast6", "tone"): 1.275e-06,
    ("mixed", "noise"): 1.137e-06, ("mixed", "tone"): 3.134e-06,
    ("fast115", "noise"): 1.239e-06, ("fast115", "tone"): 1.729e-06,
    ("slow6", "noise"): 1.628e-06, ("slow6", "tone"): 1.834e-06,
    ("list", "noise"): 2.511e-07, ("list", "tone"): 2.523e-07,
    ("order6", "noise"): 1.257e-06, ("order6", "tone"): 4.102e-06,
    ("mixed25", "noise"): 1.310e-06, ("mixed25", "tone"): 2.980e-06,
    ("list25", "noise"): 3.457e-07, ("list25", "tone"): 4.343e-07,
}
STREAMED_TILES = 37                              # 41 tiles less the four end tiles, which no one pushes


@functools.lru_cache(maxsize=None)
def run_case(curve, sig):
    """(relative error, redo tiles, len_out, outputs left at the prefill value) of one case on the GPU"""
    import torch as t
    from pyaudiorestoration_amd import _dev, _lib, resampling
    st, sp, n, x, pos, want = K.case(curve, sig)
    plan = resampling.speed_plan_dev(t.from_numpy(np.array(st)).cuda(), t.from_numpy(np.array(sp)).cuda(), n, fused=True)
    assert plan.fused_ok
    out = t.full((plan.len_out,), 7.0, dtype=t.float32, device="cuda")
    resampling.varispeed_fused_dev(plan, t.from_numpy(np.array(x)).cuda(), K.NT, out)
    redo = ctypes.c_int(-1)
    _lib.check(_lib.lib().par_fused_redo_tiles(0, _dev.ptr(plan.aux), plan.max_out, plan.m, ctypes.byref(redo), _dev.stream_ptr(0)))
    got = out.cpu().numpy()
    if len(got) != len(want):
        return None, redo.value, len(got), None
    err = float(np.float64(np.max(np.abs(got.astype(np.float64) - want))) / float(np.max(np.abs(want))))
    return err, redo.value, len(got), int(np.count_nonzero(got == 7.0))


@pytest.mark.parametrize("sig", K.SIGNALS)
@pytest.mark.parametrize("curve", K.CURVES)
def test_hot_loops_against_the_oracle(curve, sig):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    want = K.case(curve, sig)[5]
    err, redo, n_out, left = run_case(curve, sig)
    print(f"{curve:7s} {sig:5s} err {err!r} redo {redo} len_out {n_out} left {left}")
    assert n_out == len(want), (curve, sig, n_out, len(want))
    assert left == 0, (curve, sig, left)
    if curve == "list25":
        assert 0 < redo < STREAMED_TILES, (curve, sig, redo)
    elif curve == "mixed":                       # (the cubic flanks: see the head of this file)
        assert 0 < redo < STREAMED_TILES, (curve, sig, redo)
    elif curve == "list":
        assert run_case("mixed", sig)[1] < redo < STREAMED_TILES, (curve, sig, redo, run_case("mixed", sig)[1])
    else:
        assert redo == 0, (curve, sig, redo)
    assert err < TOL, (curve, sig, err)
    assert err <= 1.25 * PARENT[(curve, sig)], (curve, sig, err, PARENT[(curve, sig)])
