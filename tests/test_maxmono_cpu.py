"""MaxMono without a GPU: the numpy statement over the oracle's STFT / ISTFT against the reference's own results
(tests/golden/maxmono.npz, written by tools/gen_golden_maxmono.py), the preconditions of the GPU tests' inputs, the power of the
fused-against-composed test, and the host side of pyaudiorestoration_amd.dropouts.  pytest -s prints the measured figures."""
import os

import numpy as np
import pytest

import maxmono_inputs as I
import maxmono_np as M
import stft_np as N
from test_renoiser_gpu import FUSED_TOL          # the project's fused-against-composed figure, 1e-6 of the peak

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# The oracle's STFT transforms the same float32 frames as the reference's numpy backend and its ISTFT sums in float64, so what is
# left is the order of float64 operations (the reference transforms frame by frame above 512 points, the oracle all frames at
# once) and the cast of the written file to float32: half a float32 ulp of the output, 6e-8 of the peak.  Measured: 0 mask bits
# differ at the three settings and the outputs differ by at most 4.7e-8 of the peak (the cast alone).
GOLDEN_TOL = 1.2e-7            # one float32 ulp at the peak


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "maxmono.npz"))


@pytest.fixture(scope="module")
def fixture_stereo(gold):
    from pyaudiorestoration_amd import io_ops
    sig, sr, _ = io_ops.read_file(os.path.join(GOLDEN, "nr_signal.wav"))
    sig = sig if sig.ndim == 2 else sig[:, None]
    assert float(np.sum(sig, dtype=np.float64)) == float(gold["signal_sum"])
    return np.concatenate([sig, np.roll(sig, int(gold["stereo_shift"]), axis=0)], axis=1).astype(np.float32)


def test_fixture_records_a_float64_transform(gold):
    assert str(gold["spec_dtype"]) == "complex128" and list(gold["backend"]) == ["np_rfft_pick"]
    assert [tuple(s) for s in gold["settings"]] == [(2048, 512), (512, 64), (64, 16)]
    assert os.path.getsize(os.path.join(GOLDEN, "maxmono.npz")) < 1 << 20


def test_numpy_statement_reproduces_the_reference(gold, fixture_stereo):
    from oracle import oracle_np
    stride = int(gold["stride"])
    for fft, hop in gold["settings"]:
        fft, hop = int(fft), int(hop)
        k = f"{fft}_{hop}"
        y_max, y_min, m_max, m_min = M.max_mono(fixture_stereo, fft, hop, oracle_np.stft, oracle_np.istft)
        frames, bins = int(gold[f"{k}_frames"]), fft // 2 + 1
        assert m_max.shape == (bins, frames)
        for op, y, m in (("max", y_max, m_max), ("min", y_min, m_min)):
            ref_m = M.unpack_mask(gold[f"{k}_mask_{op}"], frames, bins)
            differ = int(np.sum(m.T != ref_m))
            peak = float(gold[f"{k}_peak_{op}"])
            err = float(np.max(np.abs(np.asarray(y, np.float64)[::stride] - gold[f"{k}_y_{op}"].astype(np.float64)))) / peak
            print(f"\n{fft}/{hop} {op}: {differ} of {ref_m.size} mask bits differ, output {err:.2e} of the peak", end="")
            assert differ == 0, (fft, hop, op, differ)
            assert len(y) == len(fixture_stereo) and err <= GOLDEN_TOL, (fft, hop, op, err)
        assert not (m_max & m_min).any()


def test_tie_spectra_hold_ties_and_their_neighbours():
    c = I.tie_spectra()
    assert c.L.dtype == c.R.dtype == np.complex64 and c.L.shape[1] > 4 * 256 and c.L.shape[1] % 2 == 1
    a, b = np.abs(c.L), np.abs(c.R)
    assert a.dtype == np.float32 and np.isfinite(a).all() and (a > 0).all()
    assert np.array_equal(a[c.cls == 0], b[c.cls == 0])                                       # ties
    assert np.array_equal(np.nextafter(a[c.cls == 1], -I.INF32), b[c.cls == 1])               # |R| one ulp under |L|
    assert np.array_equal(np.nextafter(a[c.cls == 2], I.INF32), b[c.cls == 2])                # ... one ulp over
    assert (c.cls[0] == 0).all()                                                              # every bin of row 0 a tie
    counts = [int((c.cls[1:] == k).sum()) for k in range(3)]
    assert min(counts) >= c.L.shape[1], counts                                                # each class populated beyond row 0
    assert (c.R.real != 0).any() and (c.R.imag != 0).any() and (c.R.real < 0).any() and (c.R.imag < 0).any()
    d_max, d_min = M.select(c.L, c.R)
    tie, under, over = c.cls == 0, c.cls == 1, c.cls == 2
    assert np.array_equal(I.bits(d_max)[tie], I.bits(c.R)[tie]) and np.array_equal(I.bits(d_min)[tie], I.bits(c.R)[tie])
    assert np.array_equal(I.bits(d_max)[under], I.bits(c.L)[under]) and np.array_equal(I.bits(d_min)[under], I.bits(c.R)[under])
    assert np.array_equal(I.bits(d_max)[over], I.bits(c.R)[over]) and np.array_equal(I.bits(d_min)[over], I.bits(c.L)[over])
    # a >= slip takes L on every tie: it would show in every tie whose L and R differ, which is all of them
    assert (c.L[tie] != c.R[tie]).all()
    print(f"\ntie spectra {c.L.shape}: {int(tie.sum())} ties, {counts[1]} an ulp under, {counts[2]} an ulp over")


def test_near_tie_excusal_is_narrow():
    """what the fused test may excuse: ties and their ulp neighbours are near, independent spectra almost never are, and one
    near bin takes one frame's reach out of the comparison"""
    c = I.tie_spectra()
    assert M.near_ties(c.L, c.R).all()
    f = I.free_spectra(200, 257, 3)
    near = M.near_ties(f.L, f.R)
    assert near.sum() <= 5e-5 * near.size, int(near.sum())
    one = np.zeros((40, 33), bool)
    one[10, 5] = True
    ok = M.unreached(one, 16, 64, 600)
    assert (~ok).sum() == 64 and not ok[10 * 16 - 32] and not ok[10 * 16 + 31] and ok[10 * 16 - 33] and ok[10 * 16 + 32]


def test_special_spectra_hold_every_pair_of_parts():
    c = I.special_spectra()
    p = len(I.PARTS)
    assert c.L.shape == c.R.shape == (p * p, p * p)
    seen = {(z.real.tobytes(), z.imag.tobytes()) for z in c.L[:, 0]}
    assert len(seen) == p * p and seen == {(z.real.tobytes(), z.imag.tobytes()) for z in c.R[0]}
    assert np.isnan(I.NAN_A) and np.isnan(I.NAN_B) and I.bits(np.array([I.NAN_A]))[0] != I.bits(np.array([I.NAN_B]))[0]
    assert I.is_denormal(c.L.real).any() and I.is_denormal(c.R.imag).any()
    d_max, d_min = M.select(c.L, c.R)
    with np.errstate(invalid="ignore"):
        a, b = np.abs(c.L), np.abs(c.R)
    nan = np.isnan(a) | np.isnan(b)
    assert nan.any() and np.array_equal(I.bits(d_max)[nan], I.bits(c.R)[nan]) and np.array_equal(I.bits(d_min)[nan], I.bits(c.R)[nan])
    both_inf = np.isinf(a) & np.isinf(b)
    assert both_inf.any() and np.array_equal(I.bits(d_max)[both_inf], I.bits(c.R)[both_inf])  # inf against inf is a tie
    # np.where moved bits: payloads, signed zeros and denormals arrive as they left
    took_l = a > b
    assert np.array_equal(I.bits(d_max)[took_l], I.bits(c.L)[took_l]) and I.is_denormal(d_min.real).any()
    assert (I.bits(d_max.real.copy()) == I.bits(np.array([I.NAN_A]))[0]).any()
    assert (I.bits(d_min.real.copy()) == 0x80000000).any()                                    # -0.0
    print(f"\nspecial spectra: {c.L.size} cells, {int(nan.sum())} with a NaN magnitude, {int(both_inf.sum())} inf against inf")


def test_restated_geometry_and_lengths():
    assert I.largest_fused_hop(8192) == 5114 and not I.supported(8192, 5115) and I.supported(8192, 5114)
    for n_fft in (16, 64, 512, 2048, 4096):
        assert I.largest_fused_hop(n_fft) == n_fft
    assert not I.supported(16384, 4096) and not I.supported(8, 2) and not I.supported(1000, 250) and not I.supported(512, 513)
    assert {s[0] for s in I.FUSED_SIZES} == {1 << k for k in range(4, 14)}
    for n_fft, hop in I.FUSED_SIZES:
        assert I.supported(n_fft, hop), (n_fft, hop)
        ls = I.lengths(n_fft, hop)
        assert ls[0] < n_fft // 2 and I.runs(ls[1], n_fft, hop) == 1 and ls[2] == 25 * n_fft + 1
        assert max(I.runs(n, n_fft, hop) for n in ls) >= 3, (n_fft, hop)
        last = max(ls)
        assert (last + n_fft // 2) % I.run_samples(n_fft, hop) != 0                           # a ragged end


@pytest.mark.parametrize("n_fft,hop", I.FUSED_SIZES)
def test_one_flipped_decision_is_ten_tolerances(n_fft, hop):
    """The power of the fused-against-composed test, on its own inputs: taking the other channel in ONE bin -- of median
    |D_L - D_R| in an interior frame -- moves the max output by at least 10 x FUSED_TOL of its peak.  Measured: 6.8e-4 of the
    peak at 8192/2048 (the smallest), up to 8.3e-2 at 64/64; identical masks leave rounding only."""
    n = max(I.lengths(n_fft, hop))
    x = I.stereo(n, n_fft + hop)
    w = N.window32("blackmanharris", n_fft)
    half = n_fft // 2
    pad = np.zeros((n + half, 2), np.float32)
    pad[:n] = x
    SL, SR = N.stft64(pad[:, 0], n_fft, hop, 1, w), N.stft64(pad[:, 1], n_fft, hop, 1, w)
    keep = min(len(SL), -(-(n + n_fft) // hop))
    SL, SR = SL[:keep], SR[:keep]
    d_max, _ = M.select(SL, SR)
    y = N.istft64(d_max, n_fft, hop, w, n, half).y
    peak = float(np.max(np.abs(y)))
    f = keep // 2
    b = M.median_bin(SL, SR, f)
    delta = np.zeros_like(d_max)
    delta[f, b] = (SR[f, b] if d_max[f, b] == SL[f, b] else SL[f, b]) - d_max[f, b]
    moved = float(np.max(np.abs(N.istft64(delta, n_fft, hop, w, n, half).y)))              # the ISTFT is linear
    print(f"\n{n_fft}/{hop}: n {n}, frame {f} bin {b}: one flip moves the output by {moved / peak:.2e} of the peak", end="")
    assert moved >= 10 * FUSED_TOL * peak, (n_fft, hop, moved / peak)


def test_host_helpers_and_argument_errors():
    from pyaudiorestoration_amd import dropouts
    assert dropouts.output_paths("/a/b/tape.wav") == ("/a/b/tapemax.wav", "/a/b/tapemin.wav")
    assert dropouts.output_paths("tape.x.flac") == ("tape.xmax.wav", "tape.xmin.wav")
    assert (dropouts.FFT_SIZE, dropouts.OVERLAP, dropouts.WINDOW) == (512, 4, "blackmanharris")
    for n_fft, hop in I.FUSED_SIZES + ((8192, 5115), (16384, 4096), (8, 2), (1000, 250), (512, 513), (512, 0)):
        assert dropouts.fused_supported(n_fft, hop) == I.supported(n_fft, hop), (n_fft, hop)
        assert dropouts.FUSED(n_fft, hop) in (True, False)
        assert not (dropouts.FUSED(n_fft, hop) and not dropouts.fused_supported(n_fft, hop))
    x = np.zeros((100, 2), np.float32)
    with pytest.raises(ValueError, match="stereo"):
        dropouts.max_mono(x[:, 0])
    with pytest.raises(ValueError, match="stereo"):
        dropouts.max_mono(x[:, :1])
    with pytest.raises(ValueError, match="stereo"):
        dropouts.max_mono(np.zeros((100, 3), np.float32))
    with pytest.raises(ValueError, match="fft_size"):
        dropouts.max_mono(x, fft_size=511)
    with pytest.raises(ValueError, match="hop"):
        dropouts.max_mono(x, hop=0)
    with pytest.raises(ValueError, match="channels"):
        dropouts.max_mono(x, channels=(0,))
    with pytest.raises(IndexError):
        dropouts.max_mono(x, channels=(0, 2))
    with pytest.raises(ValueError, match="one shape"):
        dropouts.select_spectra(np.zeros((3, 4), np.complex64), np.zeros((4, 3), np.complex64))
    with pytest.raises(ValueError, match="expects stereo"):
        dropouts.process("mono.wav", signal_data=(np.zeros((100, 1), np.float32), 44100, 1))
