"""CPU checks of the harmonic / percussive separation port: the tests' numpy / scipy statement (tests/hpss_np.py) against the
reference's own results on the stored spectrogram crop (tests/golden/hpss.npz, written by tools/gen_golden_hpss.py), the reflect
rule, the argument errors that need no GPU, the public signatures and the `hpss` subcommand's parser.  No GPU needed."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import hpss_inputs
import hpss_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# S * mask (what the kernel and hpss_np.hpss compute) against the reference's (|S| * mask) * exp(i angle(S)), relative to the
# modulus: the float32 angle is off by up to 2^-24 * pi = 1.9e-7 rad, cos and sin by up to an ulp each (1.7e-7 of the modulus
# together), |S|, |S| * mask and the product with the phasor round once each (3 x 6e-8), S * mask itself once (6e-8)
PHASOR_REL = 6e-7


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "hpss.npz"))


def test_fixture_present_small_and_complete(gold):
    assert os.path.getsize(os.path.join(GOLDEN, "hpss.npz")) <= 1 << 20
    assert set(gold["settings"]) == {"default", "even", "k99", "k1", "power1", "margin", "stereo", "big", "short"}
    assert list(gold["backend"]) == ["np_rfft_pick"]
    for k in gold["settings"]:
        fft, hop, kh, kp, power, mh, mp, stride, residual = gold[f"{k}_params"]
        assert (f"{k}_R" in gold.files) == bool(residual) == (k == "margin")
        assert gold[f"{k}_H"].shape == gold[f"{k}_P"].shape and gold[f"{k}_H"].dtype == np.float32
    assert tuple(gold["even_params"][2:4]) == (17, 64) and tuple(gold["k99_params"][2:4]) == (99, 99) and tuple(gold["k1_params"][2:4]) == (1, 1)
    assert gold["power1_params"][4] == 1 and tuple(gold["margin_params"][5:7]) == (2, 3) and gold["big_params"][0] == 16384
    assert gold["stereo_H"].shape[1] == 2
    n_short, fft, hop, kh = int(gold["short"]), *(int(v) for v in gold["short_params"][:3])
    assert (n_short + fft // 2) // hop + 1 < kh // 2                    # fewer frames than the median's halo
    assert gold["crop_S"].dtype == np.complex64 and gold["crop_S"].shape == gold["crop_H"].shape == gold["crop_harm"].shape


def test_closed_form_input_is_the_one_the_fixture_was_made_from(gold):
    x = hpss_inputs.tones_bursts_silence()
    assert x.dtype == np.float32 and float(np.sum(x, dtype=np.float64)) == float(gold["synth_sum"])
    lo, hi = (int(t * hpss_inputs.SR) for t in hpss_inputs.SILENCE)
    assert not x[lo:hi].any() and (hi - lo) // 128 > 99 + 4             # exact silence, longer than the widest window of frames


def test_numpy_statement_reproduces_the_reference_medians_and_masks_exactly(gold):
    S = gold["crop_S"]
    harm, perc = hpss_np.medians(np.abs(S), 31, 31)
    assert np.array_equal(harm, gold["crop_harm"]) and np.array_equal(perc, gold["crop_perc"])
    mh, mp = hpss_np.masks(np.abs(S))
    assert mh.dtype == np.float32 and np.array_equal(mh, gold["crop_mask_h"]) and np.array_equal(mp, gold["crop_mask_p"])
    both_small = np.maximum(harm, perc) < hpss_np.TINY
    assert both_small.sum() > 48 * 31 and (mh[both_small] == 0.5).all() and (mp[both_small] == 0.5).all()
    hard = hpss_np.masks(np.abs(S), power=np.inf)
    assert np.array_equal(np.packbits(np.stack(hard)), gold["crop_hard"])
    # decompose.harmonic on magnitudes with an even kernel, power 1 and two margins (bad entries -> 0), softmask called directly
    kh, kp, power, m_h, m_p = gold["crop_harmonic_params"]
    hh, pp = hpss_np.medians(np.abs(S), int(kh), int(kp))
    assert np.array_equal(np.abs(S) * hpss_np.mask(hh, pp * np.float32(m_h), power, False), gold["crop_harmonic"])
    assert np.array_equal(hpss_np.mask(harm, perc * np.float32(1.5), 3, True), gold["crop_softmask"])


def test_numpy_statement_reproduces_the_reference_components(gold):
    S = gold["crop_S"]
    # the reference's order of operations: within 1 ulp of float32, every real and imaginary part
    H, P = hpss_np.hpss_polar(S)
    assert H.dtype == np.complex64
    assert hpss_np.ulp_distance(H, gold["crop_H"]) <= 1 and hpss_np.ulp_distance(P, gold["crop_P"]) <= 1
    # S * mask, the product the kernel forms: the same numbers up to the rounding of the reference's phasor
    for ours, ref in zip(hpss_np.hpss(S), (gold["crop_H"], gold["crop_P"])):
        assert ours.dtype == np.complex64
        mod = np.abs(ref).astype(np.float64)
        err = np.abs(ours.astype(np.complex128) - ref)
        assert np.all(err <= PHASOR_REL * mod), float(np.max(err[mod > 0] / mod[mod > 0]))


def test_reflect_indices_equal_numpy_symmetric_padding():
    for n in range(1, 6):
        base = np.arange(n)
        for k in list(range(1, 12)) + [30, 31, 64, 98, 99]:
            left, right = k // 2, k - 1 - k // 2
            padded = np.pad(base, (left, right), mode="symmetric")
            want = np.stack([padded[i:i + k] for i in range(n)])
            assert np.array_equal(hpss_np.reflect_indices(n, k), want), (n, k)
    # ... and the selection built on it equals scipy's filter, over-long halos and even sizes included.  (Only while the halo
    # k // 2 stays under four axis lengths: past that, scipy's own index arithmetic reaches element -1 -- NOTES.md, HPSS.)
    rng = np.random.default_rng(109)
    for shape, k, axis in (((3, 7), 9, 0), ((5, 4), 31, 1), ((5, 13), 99, 1), ((33, 10), 64, 0), ((6, 40), 17, 1), ((1, 1), 31, 0),
                           ((8, 8), 2, 1)):
        a = rng.random(shape).astype(np.float32)
        harm, perc = hpss_np.medians(a, k, k)
        assert np.array_equal(hpss_np.median_reflect(a, k, axis), perc if axis == 0 else harm), (shape, k, axis)


def test_abi_argument_errors_need_no_gpu():
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    assert L.par_version() == 109
    p = [ctypes.c_void_p(v) for v in (64, 128, 192)]

    def call(spec=p[0], is_complex=1, frames=10, bins=33, pitch=0, kh=31, kp=31, power=2.0, mh=1.0, mp=1.0, out_h=p[1], out_p=p[2], kind=0):
        return L.par_hpss_f32(0, spec, is_complex, frames, bins, pitch, kh, kp, power, mh, mp, out_h, out_p, kind, None)
    for kw, word in ((dict(kh=0), "kernel sizes"), (dict(kp=100), "kernel sizes"), (dict(kh=-3), "kernel sizes"), (dict(power=0.0), "power"),
                     (dict(power=-1.0), "power"), (dict(power=float("nan")), "power"), (dict(mh=0.99), "margins"), (dict(mp=0.0), "margins"),
                     (dict(spec=None), "null"), (dict(out_h=None), "null"), (dict(out_p=None), "null"), (dict(out_p=None, kind=1), "null"),
                     (dict(kind=4), "out_kind"), (dict(out_h=p[0]), "in place"), (dict(bins=0), "bad sizes"), (dict(pitch=20), "bad sizes"),
                     (dict(frames=-1), "bad sizes")):
        assert call(**kw) == 1 and word in _lib.last_error(), (kw, _lib.last_error())
    assert call(frames=0) == 0                                          # nothing to do: no device is touched
    assert call(frames=0, out_p=None, kind=_lib.HPSS_HARMONIC) == 0     # the harmonic form needs no second output
    assert L.par_residual_f32(0, None, 1, p[0], 1, p[1], 1, 5, p[2], 1, None) == 1 and "null" in _lib.last_error()
    assert L.par_residual_f32(0, p[0], 0, p[0], 1, p[1], 1, 5, p[2], 1, None) == 1 and "bad sizes" in _lib.last_error()
    assert L.par_residual_f32(0, p[0], 1, p[0], 1, p[1], 1, 0, p[2], 1, None) == 0


def test_python_argument_errors_before_any_device_work():
    from pyaudiorestoration_amd import decompose, hpss
    S = np.zeros((33, 5), np.complex64)
    for kw in (dict(power=0), dict(power=-2.0), dict(margin=0.5), dict(margin=(1.0, 0.9)), dict(kernel_size=0), dict(kernel_size=(31, 100)),
               dict(kernel_size=2.5)):
        with pytest.raises(ValueError):
            decompose.hpss(S, **kw)
        with pytest.raises(ValueError):
            decompose.harmonic(S, **kw)
    with pytest.raises(ValueError):
        decompose.softmask(np.ones(3), np.ones(4))
    with pytest.raises(ValueError):
        decompose.softmask(np.ones(3), -np.ones(3))
    with pytest.raises(ValueError):
        decompose.softmask(np.ones(3), np.ones(3), power=0)
    assert hpss.has_residual(1.0) is False and hpss.has_residual(1.5) and hpss.has_residual((1.0, 1.0))
    assert hpss.output_paths("/a/b/take.flac") == ["/a/b/take_H.wav", "/a/b/take_P.wav"]
    assert hpss.output_paths("/a/b/take.flac", (2.0, 3.0))[-1] == "/a/b/take_R.wav"


def test_softmask_is_the_reference_rule(gold):
    from pyaudiorestoration_amd import decompose
    harm, perc = gold["crop_harm"], gold["crop_perc"]
    assert np.array_equal(decompose.softmask(harm, perc * np.float32(1.5), power=3, split_zeros=True), gold["crop_softmask"])
    assert np.array_equal(decompose.softmask(harm, perc, power=2.0, split_zeros=True), gold["crop_mask_h"])
    hard = np.stack([decompose.softmask(harm, perc, power=np.inf), decompose.softmask(perc, harm, power=np.inf)])
    assert hard.dtype == bool and np.array_equal(np.packbits(hard), gold["crop_hard"])
    assert decompose.softmask(np.array([1, 0]), np.array([3, 0])).dtype == np.float32                # integers are computed in float32
    assert np.array_equal(decompose.softmask(np.array([1, 0]), np.array([3, 0])), np.float32([0.25, 0.0]))
    mag, phase = decompose.magphase(gold["crop_S"])
    assert mag.dtype == np.float32 and np.array_equal(mag, np.abs(gold["crop_S"]))


def test_public_signatures_match_the_reference(gold):
    from pyaudiorestoration_amd import decompose, hpss
    ours = []
    for name in ("hpss", "harmonic", "softmask"):
        pars = inspect.signature(getattr(decompose, name)).parameters.values()
        ours.append(name + ":" + ",".join(p.name if p.default is inspect.Parameter.empty else f"{p.name}={p.default!r}" for p in pars))
    assert ours == list(gold["signatures"])
    E = inspect.Parameter.empty
    assert [(p.name, p.default) for p in inspect.signature(hpss.separate).parameters.values()] == [
        ("signal", E), ("sr", E), ("fft_size", 512), ("hop", 128), ("kernel", (31, 31)), ("power", 2.0), ("margin", 1.0), ("channels", None)]


def test_cli_hpss_parsing():
    from pyaudiorestoration_amd import cli
    a = cli.parser().parse_args(["hpss", "x.wav", "y.flac"])
    assert (a.cmd, a.fft, a.overlap, a.kernel, a.power, a.margin, a.files) == ("hpss", 512, 4, (31, 31), 2.0, 1.0, ["x.wav", "y.flac"])
    a = cli.parser().parse_args(["hpss", "--fft", "2048", "--overlap", "8", "--kernel", "17,64", "--power", "inf", "--margin", "2,3", "x.wav"])
    assert (a.fft, a.overlap, a.kernel, a.margin) == (2048, 8, (17, 64), (2.0, 3.0)) and np.isinf(a.power)
    a = cli.parser().parse_args(["hpss", "--kernel", "9", "--margin", "1.5", "x.wav"])
    assert a.kernel == 9 and a.margin == 1.5
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["hpss", "--kernel", "1,2,3", "x.wav"])
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["hpss"])
