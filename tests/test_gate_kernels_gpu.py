"""The renoiser's two gate entry points (csrc/stft.hip, ABI 108) at the C ABI against numpy, with the cutoffs ON the magnitudes
(tests/gate_inputs.py): a bin passes when float32(np.abs(X)) + 1e-7f >= cutoff, so a device |X| one ulp under np.abs gates a tie
of `cut_on` and one ulp over it passes a tie of `cut_above`.  tests/test_gate_inputs_cpu.py proves the ties exist on both sides and
that a +-1 ulp magnitude in 13 % of the bins flips over 4000 decisions of case A.

par_gate_spectrum_f32: every cell of the result equals numpy's complex64 product bit for bit; the spectrum lies between guard rows
and its pitch padding holds a sentinel, all unchanged bit for bit afterwards.  Special values (case C): where numpy's product is a
NaN (inf * 0, or a NaN part) the kernel's is a NaN too, whatever its sign and payload -- those are the processor's, not numpy's;
every other cell, the float32 denormal parts included, is bit-equal: the kernel does not flush denormals, neither in |X| nor in
the product.

par_gate_stft_f32: against numpy's gate of K_stft's spectrum put through K_istft, within FUSED_TOL of the output's peak, with every
bin's median-magnitude frame a tie.  One flipped tie is worth over 100 x FUSED_TOL (computed and asserted here), so the header's
sentence "the same gate decisions as par_gate_spectrum_f32 on par_stft_f32's spectrum" is what these tests hold."""
import ctypes

import numpy as np
import pytest

import gate_inputs as G
from test_heal_kernels_gpu import Guarded, bits
from test_renoiser_gpu import FUSED_TOL, spectrum_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def par():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pyaudiorestoration_amd import _dev, _lib

    class P:
        pass
    p = P()
    p.torch, p.dev, p.L, p.check, p.stream = torch, 0, _lib.lib(), _lib.check, lambda: _dev.stream_ptr(0)
    return p


def run_gate(par, c, key, pitch=None):
    """-> (device result (frames, bins), numpy's, cells that differ as a bool array); asserts guards and padding"""
    body = c.pitched(pitch)
    spec = Guarded(par, body, 2, G.SENTINEL)
    cut = Guarded(par, c.cuts[key], 64, np.float32(np.nan))
    p = c.pitch if pitch is None else pitch
    par.check(par.L.par_gate_spectrum_f32(par.dev, spec.ptr(), c.frames, c.bins, p, cut.ptr(), float(G.LOW), par.stream()))
    par.torch.cuda.synchronize()
    got = spec.read()
    assert spec.guards_intact() and cut.unchanged(), (c, key)
    assert np.array_equal(bits(got[:, c.bins:]), bits(body[:, c.bins:])), (c, key)          # the pitch padding
    got = np.ascontiguousarray(got[:, :c.bins])
    want = G.gate_np(c.spec, c.cuts[key])
    return got, want, (bits(got) != bits(want)).reshape(c.frames, c.bins, 2).any(axis=2)


def report(c, key, got, want, diff):
    """which way the differing decisions went: numpy passes and the kernel gated, or the reverse"""
    ref_pass = G.passes_np(c.spec, c.cuts[key])
    gated = int((diff & ref_pass).sum())
    passed = int((diff & ~ref_pass).sum())
    print(f"\ncase {c.name}, cut_{key}: {int(diff.sum())} of {diff.size} cells differ from numpy's: {gated} gated where numpy passes, "
          f"{passed} passed where numpy gates; by frame {np.flatnonzero(diff.any(axis=1))[:8].tolist()}")


@pytest.mark.parametrize("key", ["on", "above"])
def test_gate_spectrum_case_a_every_bin_of_row0_a_tie(par, key):
    c = G.case_a()
    got, want, diff = run_gate(par, c, key)
    report(c, key, got, want, diff)
    assert not diff.any(), (key, int(diff.sum()), np.argwhere(diff)[:5].tolist())


@pytest.mark.parametrize("pitch", G.B_PITCHES)
@pytest.mark.parametrize("key", ["on", "above"])
def test_gate_spectrum_case_b_second_pass_of_the_frame_loop(par, key, pitch):
    c = G.case_b()
    got, want, diff = run_gate(par, c, key, pitch)
    report(c, key, got, want, diff)
    assert not diff.any(), (key, pitch, int(diff.sum()), np.argwhere(diff)[:5].tolist())


def test_gate_spectrum_case_c_special_values(par):
    c = G.case_c()
    got, want, _ = run_gate(par, c, "special")
    g, w = got.view(np.float32), want.view(np.float32)
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), np.argwhere(np.isnan(g) != nan)[:5].tolist()
    differ = (bits(got) != bits(want)) & ~nan
    den = G.is_denormal(c.spec.view(np.float32))
    print(f"\ncase C: {int(nan.sum())} NaN parts on both sides; {int(differ.sum())} other parts differ, {int((differ & den).sum())} of them "
          f"on the {int(den.sum())} denormal parts")
    # the decisions first (a gated part is scaled by 1e-3, a passing one is not), then every bit
    fin = np.isfinite(w) & (w != 0) & ~den
    assert np.array_equal(g[fin], w[fin])
    assert not differ.any(), np.argwhere(differ)[:5].tolist()


def test_gate_spectrum_argument_errors(par):
    fn, p = par.L.par_gate_spectrum_f32, ctypes.c_void_p(8)
    assert fn(par.dev, None, 3, 5, 0, p, 0.5, None) == 1 and fn(par.dev, p, 3, 5, 0, None, 0.5, None) == 1
    assert fn(par.dev, p, 3, 0, 0, p, 0.5, None) == 1 and fn(par.dev, p, -1, 5, 0, p, 0.5, None) == 1
    assert fn(par.dev, p, 3, 5, 4, p, 0.5, None) == 1                                       # pitch < bins
    assert fn(par.dev, p, 0, 5, 0, p, 0.5, None) == 0                                       # no frames: nothing to do


# ------------------------------------------------------------------------------------------ fused
def fused_case(par, n_fft, hop, n, interleaved):
    """-> (x (n, ch) float32, channel, S host (frames, bins), spectrum device tensor (frames, bins))"""
    x = G.fused_signal(n, n_fft)
    if interleaved:
        x2 = np.stack([G.fused_signal(n, n_fft + 1), x], axis=1)
        ch = 1
    else:
        x2, ch = x[:, None], 0
    fm = spectrum_dev(x, n_fft, hop, par.dev)
    return np.ascontiguousarray(x2), ch, fm.cpu().numpy().copy(), fm


def run_fused(par, x2, ch, n_fft, hop, cut):
    from pyaudiorestoration_amd import fourier
    n, n_ch = x2.shape
    x = Guarded(par, x2, 64, np.float32(7e37))
    y = Guarded(par, np.full((n, n_ch), np.float32(-1234.5)), 64, np.float32(-1234.5))
    c = Guarded(par, cut, 64, np.float32(np.nan))
    w = fourier.window_dev("blackmanharris", n_fft, par.dev)
    par.check(par.L.par_gate_stft_f32(par.dev, x.ptr(ch), n, n_ch, 1, n_fft, hop, ctypes.c_void_p(w.data_ptr()), c.ptr(), float(G.LOW),
                                      y.ptr(ch), n_ch, par.stream()))
    par.torch.cuda.synchronize()
    got = y.read().copy()
    assert y.guards_intact() and x.unchanged() and c.unchanged()
    other = [k for k in range(n_ch) if k != ch]
    assert np.all(got[:, other] == np.float32(-1234.5))                                     # the other channel's column: untouched
    return got[:, ch]


def reference_output(par, S, cut, n_fft, hop, n):
    """numpy's gate of K_stft's spectrum on the host, uploaded, through K_istft"""
    from pyaudiorestoration_amd import fourier
    gated = par.torch.from_numpy(G.gate_np(S, cut)).cuda()
    w = fourier.window_dev("blackmanharris", n_fft, par.dev)
    return fourier.istft_dev(gated.T, hop, w, length=n, dev=par.dev).cpu().numpy()


@pytest.mark.parametrize("n_fft,hop,n,interleaved", [s + (False,) for s in G.FUSED_SETTINGS] + [(512, 128, 9001, True)])
def test_gate_stft_holds_numpys_decisions_on_ties(par, n_fft, hop, n, interleaved):
    x2, ch, S, _ = fused_case(par, n_fft, hop, n, interleaved)
    cuts = G.median_cuts(S)
    for key in ("on", "above"):
        share = float(G.passes_np(S, cuts[key]).mean())
        assert 0.4 <= share <= 0.6
        ref = reference_output(par, S, cuts[key], n_fft, hop, n)
        got = run_fused(par, x2, ch, n_fft, hop, cuts[key])
        assert got.shape == ref.shape == (n,) and np.isfinite(got).all()
        peak = float(np.max(np.abs(ref)))
        err = float(np.max(np.abs(got.astype(np.float64) - ref))) / peak
        print(f"\nfused {n_fft}/{hop} n={n}{' channel 1 of 2' if interleaved else ''}, cut_{key}: {S.shape[1]} tied bins, {share:.3f} pass; "
              f"largest difference {err:.3e} of the peak")
        assert err <= FUSED_TOL, (n_fft, hop, key, err)


def test_one_flipped_tie_is_worth_a_hundred_tolerances(par):
    """The power of the fused test, computed on the CPU: the output change when one median-magnitude bin of one interior frame at
    512/128 is scaled by `low` instead of passed, relative to the output's peak."""
    import scipy.signal
    n_fft, hop, n = 512, 128, 9001
    x2, ch, S, _ = fused_case(par, n_fft, hop, n, False)
    m = G.tie_value(S)
    f = G.median_frame(m)
    interior = (f >= n_fft // hop) & (f < len(S) - 2 * n_fft // hop)
    interior[[0, -1]] = False
    assert interior.any()
    w = scipy.signal.get_window("blackmanharris", n_fft)
    peak = float(np.max(np.abs(reference_output(par, S, G.median_cuts(S)["on"], n_fft, hop, n))))
    changes = np.array([G.one_bin_output_change(S[f[k], k], k, n_fft, hop, w) for k in np.flatnonzero(interior)]) / peak
    print(f"\none flipped tie at {n_fft}/{hop}: {changes.min():.3e} .. {changes.max():.3e} of the peak over {len(changes)} bins "
          f"(FUSED_TOL {FUSED_TOL:.0e})")
    assert changes.min() > 100 * FUSED_TOL
