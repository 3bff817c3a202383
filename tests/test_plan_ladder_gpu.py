"""Every rung of the speed-curve plan's retry ladder (plan_impl, csrc/pos.hip) against the oracle, on the curves of
tests/plan_ladder_inputs.py: near-ties in the lengths on a lazy plan, on an eager one and together with a long segment (four goes), a
product outside the fixed-point range behind and in front of the trim, more offsets at or below zero than the stitch's table holds and
nearly as many, the serial path with long segments and an aux buffer, an aux buffer too small for the plan, the buffer bound on an
integer alone and beside a near-tie, and positions equally far from the file's end in the trim of a lazy plan, of an eager one and in
the checkpoint bisection of a long segment.

Positions: bit-equal to the C oracle's (lengths and `trimmed` with them) through every fill the plan admits.  What the ABI and the plan
header show -- path, fused_ok, lazy, par_last_plan_flags(), the header's flags, n_long, lazy, lazy_fail and cap -- equals the case's
expectation, which tests/test_plan_ladder_cpu.py derives from the curve without a GPU.  The resampled signal is held with the project's
own TOL and FUSED_TOL (tests/test_hip_parity.py).  pytest -s prints a line per case (NOTES.md, "The plan's ladder, rung by rung")."""
import numpy as np
import pytest

import inputs
import plan_ladder_inputs as P
from test_hip_parity import FUSED_TOL, TOL, _plan_arrays, oracle_spot, par, relerr, same_resample  # noqa: F401  (par: the fixture)

pytestmark = pytest.mark.gpu

BLOCK_NT = 16           # any NT but 32 takes the block kernel (include/par_hip.h, par_varispeed_fused_f32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _spot(out, ref, sig, NT, centre, width=1200):
    """`width` outputs around output `centre` against the C oracle's sinc at the oracle's positions"""
    from oracle import oracle_c as C
    lo = max(0, min(int(centre) - width // 2, len(ref) - width - 1))
    want = C.sinc(ref[lo:lo + width + 1], sig, NT)[:width]               # (the oracle's last output has no period of its own)
    e = relerr(out[lo:lo + width].cpu().numpy(), want)
    assert e < TOL, (centre, NT, e)


def _spot_centres(c, ref):
    """outputs to look at besides oracle_spot's spread, first and last (the last one ends on the trim)"""
    if c.spot == "zero":
        return [int(np.searchsorted(ref, 0.0))]                           # the positions cross the file's first sample here
    if c.spot is not None:                                                # both ends of the long segment among the short ones
        start = P.host_lengths(P.products(c.st, c.sp))
        return [int(start[31]), int(start[32])]
    return []


@pytest.mark.parametrize("name", list(P.CASES))
def test_ladder_rung_against_the_oracle(par, name):
    from oracle import oracle_c as C
    from pyaudiorestoration_amd import _dev, _lib
    t, R, L = par.torch, par.resampling, _lib.lib()
    c = P.CASES[name]
    m = len(c.sp)
    st_t, sp_t = t.from_numpy(c.st).cuda(), t.from_numpy(c.sp).cuda()
    sparse = c.n_in // (m - 1) > 16384            # speed_to_pos_dev plans such curves with an aux buffer, the others without
    if c.raises:
        with pytest.raises(ValueError):
            C.speed_to_pos(c.st, c.sp, c.n_in)
        for call in (lambda: R.speed_plan_dev(st_t, sp_t, c.n_in), lambda: R.speed_plan_dev(st_t, sp_t, c.n_in, fused=True),
                     lambda: R.speed_to_pos_dev(st_t, sp_t, c.n_in)):
            with pytest.raises(_lib.ParError, match="segment 49 "):
                call()
        t.cuda.synchronize()                      # nothing was left behind on the device
        return
    ref, trimmed = C.speed_to_pos(c.st, c.sp, c.n_in)
    ref_t = t.from_numpy(ref).cuda()
    kw = c.call_kwargs(len(ref))
    force = kw.get("force_host_chain", False)
    r = c.predict(len(ref))
    assert len(ref) == r["len_out"] and (c.len_out is None or len(ref) == c.len_out)

    # positions through the entry callers use, and why the plan left the device path
    info = {}
    pos = R.speed_to_pos_dev(st_t, sp_t, c.n_in, force_host_chain=force, info=info)
    flags_pos = int(L.par_last_plan_flags())
    assert pos.numel() == len(ref) and info["trimmed"] == trimmed, (pos.numel(), len(ref), info)
    assert np.array_equal(_bits(pos.cpu().numpy()), _bits(ref))
    q = P.predict(c.st, c.sp, c.n_in, fused=sparse, eager=True, force_host=int(force))
    if c.plain is not None and not sparse:
        assert (q["goes"], q["path"], q["flags"]) == tuple(c.plain)
    assert (info["path"], flags_pos & ~c.also) == (q["path"], q["flags"]), (info, flags_pos, q["goes"])

    # the fused plan: what the ABI hands back, what the header holds
    plan = R.speed_plan_dev(st_t, sp_t, c.n_in, fused=True, **kw)
    flags = int(L.par_last_plan_flags())
    hdr = _plan_arrays(plan)[0]
    fused_ok = 2 if plan.lazy else int(plan.fused_ok)
    cap = int(hdr[P.H_CAP:P.H_CAP + 2].view(np.int64)[0])
    print(f"\n{name:30s} goes {'/'.join(r['goes']):38s} path {plan.path} flags {flags:2d} fused_ok {fused_ok} n_long {hdr[P.H_N_LONG]} "
          f"n_direct {hdr[P.H_N_DIRECT]:4d} len_out {plan.len_out}; plain entry path {info['path']} flags {flags_pos}", end="")
    assert (plan.len_out, plan.trimmed) == (len(ref), trimmed)
    assert (plan.path, flags & ~c.also, fused_ok, int(hdr[P.H_N_LONG])) == (c.path, c.flags, c.fused_ok, c.n_long), r["goes"]
    assert (r["path"], r["flags"], r["fused_ok"], r["n_long"]) == (c.path, c.flags, c.fused_ok, c.n_long)     # (max_out from the oracle's length)
    assert (int(hdr[P.H_LAZY]), int(hdr[P.H_LAZY_FAIL]), int(hdr[P.H_FLAGS])) == (int(plan.lazy), 0, 0)
    assert cap == r["cap"] == int(np.mean(c.sp) * (c.st[-1] - c.st[0]) * 1.01)
    if name == "direct-many":                     # the stitch took every one of them, one real float64 add each
        assert r["nonpos"] <= hdr[P.H_N_DIRECT] <= P.K_MAX_DIRECT

    # positions from that plan, through every fill it admits
    got = t.empty(plan.len_out, dtype=t.float64, device="cuda")
    _lib.check(L.par_speed_to_pos_fill(0, _dev.ptr(sp_t), m, _dev.ptr(plan.work), _dev.ptr(got), plan.len_out, _dev.stream_ptr(0)))
    assert t.equal(got.view(t.int64), ref_t.view(t.int64))
    if fused_ok == 1:
        got.fill_(-1.0)
        _lib.check(L.par_speed_to_pos_fill_fused(0, _dev.ptr(sp_t), m, _dev.ptr(plan.work), _dev.ptr(plan.aux), plan.max_out,
                                                 _dev.ptr(got), plan.len_out, _dev.stream_ptr(0)))
        assert t.equal(got.view(t.int64), ref_t.view(t.int64))

    # the resampled signal
    sig = inputs.noise(c.n_in, seed=11)
    sig_t = t.from_numpy(sig).cuda()
    if fused_ok:
        for NT in (32, BLOCK_NT):
            out = R.varispeed_fused_dev(plan, sig_t, NT)
            assert same_resample(out, R.sinc_resample_dev(ref_t, sig_t, NT)), (name, NT)
            oracle_spot(out, ref, sig_t, NT)
            for centre in _spot_centres(c, ref):
                _spot(out, ref, sig, NT, centre)
    else:
        with pytest.raises(ValueError):
            R.varispeed_fused_dev(plan, sig_t, 32)
        out = R._resample_item(plan, (st_t, sp_t, sig_t), 32, 0)         # the batch driver's way out: the position-array path
        assert relerr(out.cpu().numpy(), C.sinc(ref, sig, 32, threads=8)) < TOL
