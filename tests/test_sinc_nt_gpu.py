"""K_sinc's generic tap loops (taps_unity / taps_general, csrc/sinc_block.h) across the tap count NT, 1 to 512, against the C
oracle at the contract's TOL: every NT of sinc_nt_inputs.NT_SET x every position regime x {noise, tone at the cutoff, Nyquist
tone, impulse train} through the position-array form; NaN / inf footprints; a strided channel; the fused form (mono, interleaved
stereo, one channel of two) on four speed curves.  32 and 50, the compile-time loops, run the same cases.  What the inputs reach
is verified without a GPU in test_sinc_nt_inputs_cpu.py.  Each test prints the worst error per (NT, regime, signal) before it
asserts.

Measured on an MI355X (worst relerr over the cases of a class; the bound is TOL = 1e-5): see NOTES.md, "Generic-NT tap loops"."""
import numpy as np
import pytest

import sinc_nt_inputs as I
from test_hip_parity import TOL, par, relerr  # noqa: F401  (par: the module's GPU fixture)
from test_sinc_tap_modes_cpu import ask_table, build_table_program

from oracle import oracle_c as C

pytestmark = pytest.mark.gpu


def resample(par, pos, sig, NT):
    return par.resampling.sinc_wrapper(pos, sig, 0, NT)


@pytest.mark.parametrize("NT", I.NT_SET)
def test_position_form_against_the_oracle(par, NT):
    bad = []
    for regime, variant in I.CASES:
        for name in I.SIGNALS:
            pos, sig = I.case_signal(name, regime, variant, NT)
            want = C.sinc(pos, sig, NT, threads=8)
            e = relerr(resample(par, pos, sig, NT), want)
            print(f"sinc_nt pos NT={NT} {regime}/{variant} {name} relerr={e:.3e}")
            if not e < TOL:
                bad.append((regime, variant, name, e))
    assert not bad, (NT, bad)


@pytest.mark.parametrize("NT", I.NT_NONFINITE)
def test_nonfinite_samples_spread_as_in_the_reference(par, NT):
    bad = []
    for regime, variant in I.NONFINITE_CASES:
        pos, len_in, fc = I.positions(regime, variant, NT)
        for kind in ("nan", "inf"):
            sig, at = I.nonfinite_signal(kind, regime, variant, NT, pos, len_in)
            want = C.sinc(pos, sig, NT)
            got = resample(par, pos, sig, NT)
            fin = np.isfinite(want)
            same = np.array_equal(np.isfinite(got), fin) and (kind != "nan" or np.array_equal(np.isnan(got), np.isnan(want)))
            e = relerr(np.where(fin, got, 0.0), np.where(fin, want, 0.0)) if same else np.inf
            print(f"sinc_nt {kind} NT={NT} {regime}/{variant} footprint={'same' if same else 'DIFFERS'} relerr={e:.3e}")
            if not (same and e < TOL):
                bad.append((regime, variant, kind, same, e))
    assert not bad, (NT, bad)


@pytest.mark.parametrize("NT", [7, 101])
def test_strided_channel(par, NT):
    t = par.torch
    for regime, variant in (("unity", 0), ("gentle", 0.99), ("steep", 0.45)):
        pos, sig = I.case_signal("noise", regime, variant, NT)
        flat = np.full(3 * len(sig), 3.0, dtype=np.float32)          # the channel at stride 3 from word 1
        flat[1::3] = sig
        out = t.full((2 * len(pos),), 7.0, dtype=t.float32, device="cuda")
        par.resampling.sinc_resample_dev(t.from_numpy(pos).cuda(), t.from_numpy(flat).cuda()[1:], NT, out, sig_stride=3,
                                         len_in=len(sig), out_stride=2)
        got = out.cpu().numpy()
        assert np.all(got[1::2] == 7.0), (NT, regime)
        e = relerr(got[0::2], C.sinc(pos, sig, NT))
        print(f"sinc_nt strided NT={NT} {regime}/{variant} relerr={e:.3e}")
        assert e < TOL, (NT, regime, e)


# ---- the fused form ---------------------------------------------------------------------------------------------------------------
_fused = {}


def fused_case(par, NT, curve):
    """One curve through the fused form, shared by the two tests below: the oracle's outputs for noise and for the tone at the
    cutoff, the mono launches, the interleaved stereo launch (left = noise, right = tone) and one channel of two; the cells
    K_sinc must not touch are checked here"""
    if (NT, curve) in _fused:
        return _fused[NT, curve]
    t, R = par.torch, par.resampling
    st, sp, n = I.fused_curve(curve, NT)
    pos, _ = C.speed_to_pos(st, sp, n)
    fc = min(float(np.min(1.0 / I.periods(pos))), 1.0)            # the lowest cutoff on the curve
    noise = I.signal("noise", "fused", 0, NT, n, fc, pos)
    tone = I.signal("cutoff", "fused", 0, NT, n, fc, pos)
    want = {"noise": C.sinc(pos, noise, NT, threads=8), "tone": C.sinc(pos, tone, NT, threads=8)}
    assert min(np.max(np.abs(w)) for w in want.values()) >= 0.1
    plan = R.speed_plan_dev(t.from_numpy(st).cuda(), t.from_numpy(sp).cuda(), n, fused=True)
    assert plan.fused_ok and plan.len_out == len(pos), (curve, plan.len_out, len(pos))
    L = plan.len_out
    mono = {"noise": R.varispeed_fused_dev(plan, t.from_numpy(noise).cuda(), NT).cpu().numpy(),
            "tone": R.varispeed_fused_dev(plan, t.from_numpy(tone).cuda(), NT).cpu().numpy()}
    inter = t.from_numpy(np.ascontiguousarray(np.stack((noise, tone), axis=1))).cuda()
    out = t.full((L + 3, 2), 7.0, dtype=t.float32, device="cuda")
    R.varispeed_fused_stereo_dev(plan, inter.reshape(-1)[0:], inter.reshape(-1)[1:], NT, out.reshape(-1)[0:], out.reshape(-1)[1:],
                                 sig_stride=2, len_in=n, out_stride=2)
    stereo = out.cpu().numpy()
    assert np.all(stereo[L:] == 7.0), (NT, curve)
    one = t.full((3 * L + 5,), 7.0, dtype=t.float32, device="cuda")       # the right channel alone, into every third cell
    R.varispeed_fused_dev(plan, inter.reshape(-1)[1:], NT, one, sig_stride=2, len_in=n, out_stride=3)
    one = one.cpu().numpy()
    assert np.all(one[1:3 * L:3] == 7.0) and np.all(one[2:3 * L:3] == 7.0) and np.all(one[3 * L:] == 7.0), (NT, curve)
    _fused[NT, curve] = want, mono, stereo[:L], one[0:3 * L:3]
    return _fused[NT, curve]


@pytest.mark.parametrize("NT", I.NT_FUSED)
def test_fused_form_against_the_oracle(par, NT):
    bad = []
    for curve in I.FUSED_CURVES:
        want, mono, stereo, one = fused_case(par, NT, curve)
        for what, got, ref in (("mono noise", mono["noise"], want["noise"]), ("mono tone", mono["tone"], want["tone"]),
                               ("stereo left", stereo[:, 0], want["noise"]), ("stereo right", stereo[:, 1], want["tone"]),
                               ("one of two", one, want["tone"])):
            e = relerr(got, ref)
            print(f"sinc_nt fused NT={NT} {curve} {what} relerr={e:.3e}")
            if not e < TOL:
                bad.append((curve, what, e))
    assert not bad, (NT, bad)


@pytest.mark.parametrize("NT", I.NT_FUSED)
def test_fused_stereo_equals_two_mono_launches(par, NT):
    """Within the 2e-6 of test_stereo_kernel_equals_two_mono_launches (test_hip_parity.py).

    From NT = 252 the two are NOT the same arithmetic: a stereo wave stages 640 samples per channel, a mono wave 1024, so every
    stereo wave computes in float64 while the mono waves (all of them up to NT = 378, the file's short last one beyond) run the
    float32 taps, and the bound measures the float32 path itself -- at n (1 - fc) = 265 on the c0.3 curve's last wave.  Worst
    measured on an MI355X: 1.6e-6 (NT = 380, sine, tone channel)."""
    bad = []
    for curve in I.FUSED_CURVES:
        want, mono, stereo, one = fused_case(par, NT, curve)
        for what, a, b in (("left", stereo[:, 0], mono["noise"]), ("right", stereo[:, 1], mono["tone"])):
            e = relerr(a, b)
            print(f"sinc_nt fused NT={NT} {curve} stereo {what} against mono relerr={e:.3e}")
            if not e < 2e-6:
                bad.append((curve, what, e))
    assert not bad, (NT, bad)


# ---- where the constant form begins, as the device shows it -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return ask_table(build_table_program(tmp_path_factory.mktemp("sinc_nt_gpu")), list(I.NT_SET))


@pytest.mark.parametrize("NT", [NT for NT in I.NT_SET if NT >= 5])
def test_constant_form_begins_where_the_table_says(par, table, NT):
    """The library's p0_from against the table program's, through what the kernel computes.  On an impulse train at period 1 and
    shift 1/8 an output is one tap weight.  A row in the constant form holds R_n's mid-range value and is off by
    constant_form_signature(n) ~ 0.109 / n^2 of the weight at this shift -- 2e-3 at n = 7, 6e-6 at n = 136 -- where a reciprocal,
    series or linear row is within float32 rounding (the linear fit's own gap is 1 / (128 n^4) <= 1.2e-6 from n = 9).  So each
    row says which side of p0_from it is on: every row below it must sit within a quarter of the signature, every row from it
    to the end of its second chunk beyond half of it."""
    p0 = table[NT][1]
    pos, sig, row = I.boundary_probe(NT)
    want = I.sinc_f64(pos, sig, NT)
    got = resample(par, pos, sig, NT).astype(np.float64)
    rows = [n for n in range(1, min(p0 + 8, NT))]
    assert all((row == n).sum() >= 2 for n in rows), NT
    wrong = []
    for n in rows:
        m = row == n
        rel = (got[m] - want[m]) / want[m]
        sig_n = float(I.constant_form_signature(n))
        ok = np.all(rel > 0.5 * sig_n) and np.all(rel < 1.5 * sig_n) if n >= p0 else np.all(np.abs(rel) < 0.25 * sig_n)
        if not ok:
            wrong.append((n, "constant" if n >= p0 else "not constant", float(rel.min()), float(rel.max()), sig_n))
    print(f"sinc_nt boundary NT={NT} p0_from={p0} rows 1..{rows[-1] if rows else 0} wrong={len(wrong)}")
    assert not wrong, (NT, p0, wrong)
