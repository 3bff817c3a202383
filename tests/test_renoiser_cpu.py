"""CPU checks of the renoiser port: the host derivation of the gate's magnitude cutoffs against numpy's float32 decibels, the
final profile against the reference's, the fixtures, the argument errors that need no GPU and the `renoise` subcommand's
parser.  No GPU needed."""
import inspect
import os

import numpy as np
import pytest

import renoiser_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ULPS = 2000


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "renoiser.npz"))


def _check_cutoffs(thr):
    from pyaudiorestoration_amd import renoiser
    cut = renoiser.gate_cutoffs(thr)
    assert cut.dtype == np.float32 and cut.shape == thr.shape
    bad = 0
    for s in range(0, len(thr), 256):
        t, c = thr[s:s + 256], cut[s:s + 256]
        fin = np.isfinite(c)
        # +-ULPS float32 neighbours of every finite cutoff (bit patterns clipped to [0, +inf]); NaN cutoffs: a ladder up to +inf
        base = np.where(fin, c, np.float32(3.0e38)).view(np.int32).astype(np.int64)
        bits = np.clip(base[:, None] + np.arange(-ULPS, ULPS + 1)[None, :], 0, 0x7F800000).astype(np.uint32)
        m = bits.view(np.float32)
        with np.errstate(invalid="ignore"):
            numpy_says = renoiser_np.db32(m).astype(np.float64) > t[:, None]
            kernel_says = m >= c[:, None]
        bad += int(np.count_nonzero(numpy_says != kernel_says))
    return cut, bad


def test_gate_cutoffs_equal_numpy_float32_decibels():
    rng = np.random.default_rng(108)
    thr = np.concatenate([rng.uniform(-140, 0, 600), rng.uniform(-300, 300, 100), [np.nan, np.inf, -np.inf, 0.0, -140.0, 1e300],
                          # thresholds sitting exactly on float32 decibel values (ties must stay gated)
                          renoiser_np.db32(rng.uniform(1e-7, 1, 64).astype(np.float32)).astype(np.float64)])
    cut, bad = _check_cutoffs(thr)
    assert bad == 0
    assert np.isnan(cut[np.isnan(thr)]).all() and np.isnan(cut[thr == np.inf]).all()
    assert cut[thr == -np.inf][0] == np.float32(1e-45)          # everything above 0 passes a -inf threshold


def test_gate_cutoffs_on_the_fixture_profiles(gold):
    thr = np.concatenate([gold[f"{k}_final"] for k in gold["settings"]])
    _, bad = _check_cutoffs(thr)
    assert bad == 0


def test_final_profile_matches_the_reference(gold):
    from pyaudiorestoration_amd import renoiser
    sr = int(gold["sr"])
    for k in gold["settings"]:
        fft, hop, gain, overhead, _ = gold[f"{k}_params"]
        got = renoiser.final_profile(gold[f"{k}_noise_profile"], sr, int(fft), gain, overhead, gold[f"{k}_curve"].tolist())
        assert got.dtype == np.float64
        assert np.array_equal(got, gold[f"{k}_final"]), k


def test_default_profile_and_factor(gold):
    from pyaudiorestoration_amd import renoiser
    assert np.array_equal(renoiser.default_profile(44100, 2048), gold["noprofile_noise_profile"])
    assert renoiser.low_factor(12.0) == np.float32(10 ** (12 / 20)) and renoiser.low_factor(12.0).dtype == np.float32
    assert renoiser.low_factor(0.0) == 1.0


def test_fixtures_present_and_small(gold):
    for name in ("renoiser.npz", "nr_signal.wav", "nr_noise.wav"):
        assert os.path.getsize(os.path.join(GOLDEN, name)) <= 1 << 20, name
    assert set(gold["settings"]) == {"default", "hop128", "gate", "big", "noprofile", "select", "stereo"}
    assert list(gold["backend"]) == ["np_rfft_pick"]
    for k in gold["settings"]:
        frames = int(gold[f"{k}_frames"])
        bins = int(gold[f"{k}_params"][0]) // 2 + 1
        assert gold[f"{k}_mask"].shape[1] == (frames * bins + 7) // 8


def test_sample_files_decode_to_the_fixture_sums(gold):
    from pyaudiorestoration_amd import io_ops
    sig, sr, ch = io_ops.read_file(os.path.join(GOLDEN, "nr_signal.wav"))
    noise, nsr, _ = io_ops.read_file(os.path.join(GOLDEN, "nr_noise.wav"))
    assert (sr, nsr, len(sig), len(noise)) == (44100, 44100, 40982, 74549)
    assert float(np.sum(sig, dtype=np.float64)) == float(gold["signal_sum"])
    assert float(np.sum(noise, dtype=np.float64)) == float(gold["noise_sum"])


def test_argument_errors_before_any_device_work():
    from pyaudiorestoration_amd import renoiser
    x = np.zeros(4096, np.float32)
    with pytest.raises(ValueError):
        renoiser.noise_profile(x, 48000, 44100)
    with pytest.raises(ValueError):
        renoiser.noise_profile_from_selection(x, 44100, 0.05, 0.05, 2048, 512)      # f0 == f1
    with pytest.raises(ValueError):
        renoiser.noise_profile_from_selection(x, 44100, 0.5, 0.2, 2048, 512)       # reversed
    with pytest.raises(IndexError):
        renoiser._check_channels([1], 2)                                           # y_out has one column
    with pytest.raises(ValueError):
        renoiser._check_channels([0, 0], 2)
    assert renoiser._check_channels([1, 0], 2) == [1, 0]
    with pytest.raises(ValueError):
        renoiser.final_profile(np.zeros(10, np.float32), 44100, 2048)


def test_selection_frames_follow_the_reference_rule():
    from pyaudiorestoration_amd import renoiser
    assert renoiser.selection_frames(0.1, 0.45, 44100, 512, 81) == (8, 38)
    assert renoiser.selection_frames(-1.0, 100.0, 44100, 512, 81) == (0, 80)


def test_fused_size_rule_and_redundant_frames():
    from pyaudiorestoration_amd import _lib, renoiser
    assert renoiser.fused_supported(2048, 512) and renoiser.fused_supported(8192, 8192) and renoiser.fused_supported(64, 2)
    assert not renoiser.fused_supported(16384, 4096) and not renoiser.fused_supported(2048, 4096)
    L = _lib.lib()
    n = 44100 * 600
    for fft, hop in ((2048, 512), (2048, 128), (8192, 2048), (64, 2)):
        need = (n + fft // 2 + fft) // hop
        got = L.par_gate_stft_transformed_frames(n, fft, hop)
        assert need <= got <= need * 1.10, (fft, hop, got / need)
    assert L.par_gate_stft_transformed_frames(n, 16384, 4096) == 0


def test_public_signatures():
    from pyaudiorestoration_amd import renoiser
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(renoiser.noise_profile)[:5] == [("noise", E), ("noise_sr", E), ("sr", E), ("fft_size", 2048), ("hop", 512)]
    assert sig(renoiser.noise_profile_from_selection)[:7] == [("signal", E), ("sr", E), ("t0", E), ("t1", E), ("fft_size", 2048),
                                                              ("hop", 512), ("channel", 0)]
    assert sig(renoiser.final_profile) == [("noise_profile", E), ("sr", E), ("fft_size", 2048), ("gain", 12.0), ("overhead", 3.0),
                                           ("curve", None)]
    assert sig(renoiser.gate_cutoffs) == [("final", E)]
    assert sig(renoiser.renoise) == [("signal", E), ("sr", E), ("final", E), ("gain", 12.0), ("fft_size", 2048), ("hop", 512),
                                     ("channels", None), ("device", None)]
    p = dict(sig(renoiser.renoise_file))
    assert p["noise_path"] is None and p["selection"] is None and p["signal_data"] is None and p["fft_size"] == 2048
    assert renoiser.output_path("/a/b/tape.flac", 2048) == "/a/b/tape fft=2048.wav"


def test_cli_renoise_parsing():
    from pyaudiorestoration_amd import cli
    a = cli.parser().parse_args(["renoise", "x.wav", "y.flac"])
    assert (a.cmd, a.noise, a.select, a.fft, a.overlap, a.gain, a.overhead, a.curve, a.channels, a.files) == \
        ("renoise", None, None, 2048, 4, 12.0, 3.0, None, None, ["x.wav", "y.flac"])
    a = cli.parser().parse_args(["renoise", "--select", "0.1,0.45", "--fft", "1024", "--overlap", "16", "--gain", "-20",
                                 "--curve", "1:0,3000:-6,22050:4", "--channels", "0,1", "x.wav"])
    assert a.select == [0.1, 0.45] and a.fft == 1024 and a.overlap == 16 and a.gain == -20.0
    assert a.curve == [[1.0, 0.0], [3000.0, -6.0], [22050.0, 4.0]] and a.channels == [0, 1]
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["renoise", "--noise", "n.wav", "--select", "0,1", "x.wav"])


def test_numpy_complex_magnitude_is_the_formula_the_gate_kernels_use():
    """par_gate_* compute |X| as numpy's SIMD complex64 absolute does: larger * sqrt(fma(r, r, 1)), r = smaller / larger, all
    float32 (a float64 hypot rounded once differs in about a quarter of the values).  If numpy here computed otherwise, the
    kernels' decisions would no longer be numpy's."""
    rng = np.random.default_rng(3)
    re = (rng.standard_normal(1 << 20) * 10.0 ** rng.uniform(-9, 0, 1 << 20)).astype(np.float32)
    im = (rng.standard_normal(1 << 20) * 10.0 ** rng.uniform(-9, 0, 1 << 20)).astype(np.float32)
    re[:4], im[:4] = [0, 0, 3, -0.0], [0, 2, 0, 5]
    got = np.abs((re + 1j * im).astype(np.complex64))
    hi, lo = np.maximum(np.abs(re), np.abs(im)), np.minimum(np.abs(re), np.abs(im))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(hi == 0, np.float32(0), lo / hi).astype(np.float32)
    fma = (r.astype(np.float64) * r + 1.0).astype(np.float32)          # r*r is exact in float64: one rounding as fma
    want = (np.sqrt(fma) * hi).astype(np.float32)
    assert np.array_equal(got, want)
