"""Preconditions of tests/test_gate_kernels_gpu.py, on the CPU, with numpy alone: the cutoffs of tests/gate_inputs.py put the ties
where the GPU tests say they are, on both sides of the comparison, and a magnitude that is one float32 ulp off np.abs in 13 % of the
bins -- the defect the tests exist for -- changes at least 1000 decisions of case A under either cutoff set.  pytest -s prints the
counts (NOTES.md, Renoiser)."""
import numpy as np

import gate_inputs as G


def test_low_factor_is_the_renoisers():
    from pyaudiorestoration_amd import renoiser
    assert G.LOW == renoiser.low_factor(-60) and G.LOW.dtype == np.float32


def test_case_a_ties_row0_on_either_side():
    c = G.case_a()
    assert c.spec.shape == (3, G.A_BINS) and c.spec.dtype == np.complex64 and c.pitch == G.A_PITCH >= G.A_BINS
    m = G.tie_value(c.spec)
    assert np.isfinite(m).all() and np.all(m[0] > G.EPS)                         # no zero bin: every |X| counts
    on, ab = G.passes_np(c.spec, c.cuts["on"]), G.passes_np(c.spec, c.cuts["above"])
    assert on[0].all() and on[1].all() and not on[2].any()                       # exactly rows 0 and 1 pass
    assert not ab[0].any() and ab[1].all() and not ab[2].any()                   # exactly row 1 passes
    assert np.array_equal(m[0], c.cuts["on"])                                    # every bin of row 0 is a tie: 70 001 on each side
    assert np.all(c.cuts["above"] > m[0]) and np.array_equal(np.nextafter(c.cuts["above"], -G.INF32), m[0])
    tiny = np.abs(c.spec[0, G.A_TINY])
    assert tiny.max() < 1e-6 and np.median(tiny) < 1e-7                          # the + 1e-7 dominates here
    print(f"\ncase A: {on[0].sum()} passing ties under cut_on, {(~ab[0]).sum()} gated ties under cut_above; "
          f"|X| of the tiny block {tiny.min():.2e} .. {tiny.max():.2e}")


def test_case_b_ties_each_bins_median_frame():
    c = G.case_b()
    assert c.spec.shape == (G.B_FRAMES, G.B_BINS) and G.B_FRAMES > G.GATE_GRID_ROWS          # the frame loop runs twice
    assert all(p == 0 or p >= G.B_BINS for p in G.B_PITCHES)
    m = G.tie_value(c.spec)
    f = G.median_frame(m)
    for key in ("on", "above"):
        p = G.passes_np(c.spec, c.cuts[key])
        share = float(p.mean())
        assert 0.45 <= share <= 0.55, (key, share)
        ties = int((m == c.cuts["on"][None, :]).sum())
        assert ties >= G.B_BINS
        tied_pass = p[f, np.arange(G.B_BINS)]
        assert tied_pass.all() if key == "on" else not tied_pass.any()
        second = p[G.GATE_GRID_ROWS:]                                            # the frames of the loop's second pass: both outcomes
        assert 0.4 <= float(second.mean()) <= 0.6
        print(f"\ncase B, cut_{key}: {share:.4f} of {m.size} cells pass; {ties} tied cells; behind frame {G.GATE_GRID_ROWS} "
              f"{int(second.sum())} of {second.size} cells pass")


def test_case_c_holds_the_special_values_under_every_special_cutoff():
    c = G.case_c()
    assert c.spec.shape == (G.C_FRAMES, G.C_BINS) and G.C_BINS % len(G.C_CUTS) == 0 and c.pitch > G.C_BINS
    cut = c.cuts["special"]
    seen = set()
    for r in range(G.C_FRAMES):
        for b in range(G.C_BINS):
            z = c.spec[r, b]
            seen.add((z.real.tobytes(), z.imag.tobytes(), cut[b].tobytes()))
    for re in G.C_PARTS:
        for im in G.C_PARTS:
            for k in G.C_CUTS:
                assert (re.tobytes(), im.tobytes(), k.tobytes()) in seen, (re, im, k)
    assert G.is_denormal(c.spec.real).sum() >= 3 * 4 * len(G.C_PARTS) and G.is_denormal(c.spec.imag).any()
    p = G.passes_np(c.spec, cut)
    assert not p[:, 0::4].any() and not p[:, 1::4][np.isfinite(G.tie_value(c.spec)[:, 1::4])].any()      # NaN gates all; inf all finite
    with np.errstate(invalid="ignore"):
        fin = ~np.isnan(G.tie_value(c.spec))
    assert p[:, 2::4][fin[:, 2::4]].all() and p[:, 3::4][fin[:, 3::4]].all()     # 0 and 1e-45 lie under every |X| + 1e-7
    assert not p[~fin].any()                                                     # a NaN magnitude is gated
    out = G.gate_np(c.spec, cut)
    kept = p & np.isfinite(c.spec.real) & np.isfinite(c.spec.imag)
    for part in ("real", "imag"):                                                # x * 1 - y * 0: a nonzero part survives, denormals too
        a, b = getattr(out, part)[kept], getattr(c.spec, part)[kept]
        assert np.array_equal(a[b != 0].view(np.uint32), b[b != 0].view(np.uint32))
    assert G.is_denormal(out.real[kept]).any() and G.is_denormal(out.imag[kept]).any()
    print(f"\ncase C: {int(p.sum())} of {p.size} cells pass, {int(np.isnan(out.real).sum())} real parts NaN in numpy's product")


def test_an_ulp_in_the_magnitude_changes_a_thousand_decisions_of_case_a():
    """The power of the tie construction: the gate built on np.abs moved by +-1 ulp in 13 % of the bins differs from numpy's in at
    least 1000 cells of case A under each cutoff set (an ulp down flips a passing tie of cut_on, an ulp up a gated tie of
    cut_above) -- unless the + 1e-7 absorbs the ulp, which is why the count is stated and not assumed."""
    c = G.case_a()
    mag = G.perturbed_magnitude(c.spec)
    moved = int((mag != np.abs(c.spec)).sum())
    assert 0.12 * mag.size <= moved <= 0.14 * mag.size
    for key in ("on", "above"):
        broken = (mag + G.EPS).astype(np.float32) >= c.cuts[key][None, :]
        diff = broken != G.passes_np(c.spec, c.cuts[key])
        per_row = diff.sum(axis=1)
        tiny = int(diff[0, G.A_TINY].sum())
        print(f"\ncase A, cut_{key}: {moved} magnitudes moved an ulp, {int(diff.sum())} decisions differ (rows {per_row.tolist()}), "
              f"{tiny} of them in the 4096 bins of the tiny block")
        assert diff.sum() >= 1000, (key, int(diff.sum()))
        assert per_row[1] == 0 and per_row[2] == 0                               # rows 1 and 2 are far from their cutoffs
