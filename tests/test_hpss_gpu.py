"""GPU checks of the harmonic / percussive separation port (util/decompose.py, experiments/hpss_gui.py): the kernel's medians
against scipy on K_stft's own spectrum (bit for bit), its masks against the tests' numpy statement (tests/hpss_np.py) on the same
spectrum, and the components and the tool's outputs against the reference's own results (tests/golden/hpss.npz, written by
tools/gen_golden_hpss.py).  Measured errors are printed (pytest -s) for NOTES.md."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.ndimage

import hpss_inputs
import hpss_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MASK_ULP = 6               # masks for powers other than 1, 2, 0.5 and inf, in float32 ulp: twice the measured worst (3; NOTES.md, HPSS)
SPEC_TOL = 5.0e-7          # H / P of the stored crop against the reference's, of the spectral peak: 3 x the measured 1.66e-7
OUT_TOL = 1e-5             # separate() against the reference's outputs per 4096-sample block, of the block's peak: the project's cap
#                            (3 x the measured worst, 8.5e-6 for the 99 / 99 kernels, lies above it, so the cap is the bound)
OUT_EXEMPT = "stereo"      # the one setting left out of the capped assertion: the rhythm clips have blocks 79 dB under the file's
OUT_EXEMPT_TOL = 1.9e-4    # peak, where the spectrum's rounding (it scales with the FRAMES' peak) shows: 3 x the measured 6.1e-5.
#                            The reference's own code moves by 2.4e-4 there when its spectrum is perturbed by 2e-7 of each frame's
#                            peak (NOTES.md, HPSS).  Against the file's peak the setting stays under the cap like the others.
SUM_TOL = 7.7e-7           # h + p against istft(stft(x)) for margin 1, of the peak: 3 x the measured 2.55e-7 (cap 1e-6)


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return 0


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "hpss.npz"))


@pytest.fixture(scope="module")
def sigs(gold):
    from pyaudiorestoration_amd import io_ops
    nr, sr, _ = io_ops.read_file(os.path.join(GOLDEN, "nr_signal.wav"))
    rh, _, _ = io_ops.read_file(os.path.join(GOLDEN, "rhythm.flac"))
    nr = nr if nr.ndim == 2 else nr[:, None]
    rh = rh[:, 0] if rh.ndim == 2 else rh
    a, b, n = (int(v) for v in gold["rhythm_clips"])
    synth = hpss_inputs.tones_bursts_silence()
    assert sr == int(gold["sr"])
    return {"nr": nr, "rhythm2": np.stack([rh[a:a + n], rh[b:b + n]], axis=1), "synth": synth[:, None], "short": synth[:int(gold["short"]), None]}


def setting(gold, k):
    fft, hop, kh, kp, power, mh, mp, stride, residual = gold[f"{k}_params"]
    margin = 1.0 if not residual and mh == 1 and mp == 1 else (float(mh), float(mp))
    return str(gold[f"{k}_input"]), int(fft), int(hop), (int(kh), int(kp)), float(power), margin, int(stride)


def block_relerr(a, b, block=4096, floor_db=-80):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    floor = np.max(np.abs(b)) * 10 ** (floor_db / 20)
    worst = 0.0
    for s in range(0, len(b), block):
        ref = max(float(np.max(np.abs(b[s:s + block]))), floor)
        worst = max(worst, float(np.max(np.abs(a[s:s + block] - b[s:s + block]))) / ref)
    return worst


def spectrum_dev(x, fft, hop, dev, mode=0):
    """K_stft of fix_length(x, n + fft/2): the (bins, frames) device view of the frame-major buffer"""
    import torch
    from pyaudiorestoration_amd import _dev, fourier
    xp = np.zeros(len(x) + fft // 2, np.float32)
    xp[:len(x)] = x
    return fourier.stft_dev(_dev.to_dev(xp, torch.float32, dev), fft, hop, fourier.window_dev("blackmanharris", fft, dev), 1, mode, dev=dev)


def scipy_medians(mag, kernel):
    return (scipy.ndimage.median_filter(mag, size=(1, kernel[0]), mode="reflect"),
            scipy.ndimage.median_filter(mag, size=(kernel[1], 1), mode="reflect"))


def test_medians_equal_scipy_bit_for_bit_on_k_stft_spectra(dev, gold, sigs):
    from pyaudiorestoration_amd import _dev, decompose
    cases = [setting(gold, k)[:4] for k in gold["settings"]]
    # every spectrogram height K_stft produces from 33 to 8193 bins, odd / even / unequal sizes, the extremes of both
    cases += [("nr", 64, 16, (31, 31)), ("nr", 64, 16, (99, 98)), ("nr", 128, 32, (2, 2)), ("nr", 256, 64, (1, 99)), ("synth", 1024, 256, (99, 1)),
              ("nr", 2048, 512, (64, 17)), ("nr", 4096, 1024, (98, 3)), ("synth", 8192, 2048, (5, 64)), ("synth", 16384, 4096, (99, 99)),
              ("short", 512, 64, (99, 99)), ("rhythm2", 512, 32, (31, 31)),
              ("synth", 32768, 8192, (31, 17))]           # 16385 bins from the four-step transform (par_stft_big_f32)
    checked = 0
    for src, fft, hop, kernel in cases:
        x = sigs[src]
        for c in range(x.shape[1]):
            S_dev = spectrum_dev(x[:, c], fft, hop, dev)
            mag = np.abs(_dev.to_host(S_dev))
            # scipy's own reflection is only defined while the halo stays under four axis lengths (NOTES.md, HPSS)
            assert kernel[0] // 2 < 4 * mag.shape[1] and kernel[1] // 2 < 4 * mag.shape[0]
            harm, perc = decompose.medians(S_dev, kernel)
            want_h, want_p = scipy_medians(mag, kernel)
            got_h, got_p = _dev.to_host(harm), _dev.to_host(perc)
            assert got_h.shape == mag.shape and got_h.dtype == np.float32
            assert np.array_equal(got_h.view(np.uint32), want_h.view(np.uint32)), (src, fft, hop, kernel, "harm")
            assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32)), (src, fft, hop, kernel, "perc")
            checked += mag.size
    print(f"medians: {len(cases)} settings, {checked} bins, all bit-identical to scipy.ndimage.median_filter")


def test_medians_of_float_and_pitched_and_host_input(dev, sigs):
    """float32 magnitudes (K_stft mode 1 writes them with rows pitched to 128 bytes), numpy input in either memory order"""
    from pyaudiorestoration_amd import _dev, decompose
    x = sigs["synth"][:30000, 0]
    M_dev = spectrum_dev(x, 512, 128, dev, mode=1)
    assert M_dev.T.stride(0) > M_dev.shape[0]                          # pitched rows
    mag = _dev.to_host(M_dev.T.contiguous()).T
    want_h, want_p = scipy_medians(mag, (17, 64))
    harm, perc = decompose.medians(M_dev, (17, 64))
    assert np.array_equal(_dev.to_host(harm.T.contiguous()).T, want_h) and np.array_equal(_dev.to_host(perc.T.contiguous()).T, want_p)
    for arr in (np.ascontiguousarray(mag), np.asfortranarray(mag), mag.astype(np.float64)):
        h, p = decompose.medians(arr, (17, 64))
        assert h.shape == mag.shape and np.array_equal(h, want_h) and np.array_equal(p, want_p)
    S = _dev.to_host(spectrum_dev(x, 512, 128, dev))
    h, p = decompose.medians(S.astype(np.complex128), 9)
    want_h, want_p = scipy_medians(np.abs(S), (9, 9))
    assert np.array_equal(h, want_h) and np.array_equal(p, want_p)


def test_real_input_is_read_by_magnitude(dev):
    """the bit-pattern order needs a clear sign bit: -0.0 counts as 0 (as it does for scipy), a real device tensor is read through fabs"""
    import torch
    from pyaudiorestoration_amd import _dev, decompose
    rng = np.random.default_rng(5)
    mag = rng.random((70, 90)).astype(np.float32)
    mag[rng.random(mag.shape) < 0.4] = 0.0
    signed = mag.copy()
    signed[::2, 1::3] *= np.float32(-1)                                 # negative values and -0.0
    assert np.signbit(signed[mag == 0]).any() and (signed < 0).any()
    want_h, want_p = scipy_medians(mag, (9, 6))
    harm, perc = decompose.medians(_dev.to_dev(signed.T, torch.float32, dev).T, (9, 6))
    assert np.array_equal(_dev.to_host(harm).view(np.uint32), want_h.view(np.uint32))
    assert np.array_equal(_dev.to_host(perc).view(np.uint32), want_p.view(np.uint32))
    zeros = np.where(mag == 0, np.float32(-0.0), mag)                   # numpy input: -0.0 passes the sign check
    h, p = decompose.medians(zeros, (9, 6))
    assert np.array_equal(h.view(np.uint32), want_h.view(np.uint32)) and np.array_equal(p.view(np.uint32), want_p.view(np.uint32))
    with pytest.raises(ValueError):
        decompose.medians(signed, (9, 6))


def test_medians_of_a_long_file(dev):
    """two minutes at 512/128: 41 k frames along the workgroup grid's long axis; stretches of 300 frames at both ends and inside
    are checked against scipy on a cut with 64 frames of context (the time median reaches 15)"""
    import torch
    from pyaudiorestoration_amd import _dev, decompose
    n = 44100 * 120
    g = torch.Generator(device=f"cuda:{dev}").manual_seed(9)
    x = _dev.to_host(0.1 * torch.randn(n, generator=g, device=f"cuda:{dev}"))
    S_dev = spectrum_dev(x, 512, 128, dev)
    harm, perc = decompose.medians(S_dev, (31, 17))
    frames = S_dev.shape[1]
    assert frames == (n + 256) // 128 + 1
    for lo in (0, 4000, frames // 2 - 77, frames - 300):
        a, b = max(lo - 64, 0), min(lo + 364, frames)
        mag = np.abs(_dev.to_host(S_dev[:, a:b].T.contiguous()).T)
        want_h, want_p = scipy_medians(mag, (31, 17))
        hi = min(lo + 300, frames)
        got_h = _dev.to_host(harm[:, lo:hi].T.contiguous()).T
        got_p = _dev.to_host(perc[:, lo:hi].T.contiguous()).T
        assert np.array_equal(got_h, want_h[:, lo - a:hi - a]) and np.array_equal(got_p, want_p[:, lo - a:hi - a]), lo


def test_masks_against_numpy_on_the_same_spectrum(dev, gold, sigs):
    from pyaudiorestoration_amd import _dev, decompose
    worst = {}
    for src, fft, hop, kernel in (("synth", 512, 128, (31, 31)), ("nr", 2048, 512, (17, 64)), ("short", 512, 128, (31, 31))):
        S_dev = spectrum_dev(sigs[src][:, 0], fft, hop, dev)
        mag = np.abs(_dev.to_host(S_dev))
        for power in (2.0, np.inf, 1.0, 0.5, 3.0, 1.5, 0.3, 7.0):
            for margin in ((1.0, 1.0), (2.0, 3.0), (1.1, 1.0)):
                mh, mp = decompose.hpss(S_dev, kernel, power, True, margin)
                got = [_dev.to_host(m) for m in (mh, mp)]
                want = hpss_np.masks(mag, kernel, power, margin)
                harm, perc = hpss_np.medians(mag, *kernel)
                small = np.maximum(harm, perc * np.float32(margin[0])) < hpss_np.TINY
                for g, w, name in zip(got, want, "hp"):
                    assert g.dtype == w.dtype and g.shape == w.shape
                    if power in (2.0, np.inf, 1.0, 0.5):
                        assert np.array_equal(g, w), (src, power, margin, name)
                    else:
                        d = hpss_np.ulp_distance(g, w)
                        worst[power] = max(worst.get(power, 0), d)
                        assert d <= MASK_ULP, (src, power, margin, name, d)
                if src == "synth" and np.isfinite(power):                 # the silent stretch: the Z < tiny branch, exactly
                    assert small.sum() > 100 * 257
                    value = 0.5 if margin == (1.0, 1.0) else 0.0
                    assert (got[0][small] == value).all() and np.array_equal(got[0][small], want[0][small])
    print("masks: exact for powers 2, inf, 1 and 0.5; worst float32 ulp distance by power:", worst)


def test_components_against_the_reference_crop(dev, gold):
    """the stored crop is a spectrogram of its own: medians, masks and hard masks must be the reference's bit for bit, H and P
    (S x mask here, (|S| x mask) x phasor there) agree to the rounding of the reference's phasor"""
    from pyaudiorestoration_amd import decompose
    S = gold["crop_S"]
    harm, perc = decompose.medians(S)
    assert np.array_equal(harm, gold["crop_harm"]) and np.array_equal(perc, gold["crop_perc"])
    mh, mp = decompose.hpss(S, mask=True)
    assert mh.dtype == np.float32 and np.array_equal(mh, gold["crop_mask_h"]) and np.array_equal(mp, gold["crop_mask_p"])
    hh, hp = decompose.hpss(np.asfortranarray(S), power=np.inf, mask=True)
    assert hh.dtype == bool and np.array_equal(np.packbits(np.stack([hh, hp])), gold["crop_hard"])
    H, P = decompose.hpss(S)
    assert H.dtype == np.complex64 and H.shape == S.shape
    want = hpss_np.hpss(S)
    assert np.array_equal(H, want[0]) and np.array_equal(P, want[1])          # the same products numpy forms
    peak = float(np.max(np.abs(S)))
    err = max(float(np.max(np.abs(H.astype(np.complex128) - gold["crop_H"]))), float(np.max(np.abs(P.astype(np.complex128) - gold["crop_P"])))) / peak
    print(f"crop: H / P against the reference {err:.3e} of the spectral peak")
    assert err <= SPEC_TOL
    # decompose.harmonic on magnitudes: even percussive kernel, power 1, two margins -- float32 products of exact masks
    kh, kp, power, m_h, m_p = gold["crop_harmonic_params"]
    Hm = decompose.harmonic(np.abs(S), kernel_size=(int(kh), int(kp)), power=power, margin=(m_h, m_p))
    assert Hm.dtype == np.float32 and np.array_equal(Hm, gold["crop_harmonic"])
    assert np.array_equal(decompose.harmonic(S), H)


def test_separate_against_the_reference_outputs(dev, gold, sigs):
    from pyaudiorestoration_amd import hpss
    sr = int(gold["sr"])
    worst_all = 0.0
    for k in gold["settings"]:
        src, fft, hop, kernel, power, margin, stride = setting(gold, k)
        x = sigs[src]
        h, p, r = hpss.separate(x, sr, fft, hop, kernel, power, margin)
        assert h.shape == p.shape == x.shape and h.dtype == np.float32 and (r is None) == (f"{k}_R" not in gold.files)
        worst = {}
        for name, y in (("_H", h), ("_P", p), ("_R", r)):
            if y is None:
                continue
            assert np.isfinite(y).all()
            for c in range(x.shape[1]):
                e = block_relerr(y[::stride, c], gold[f"{k}{name}"][:, c], max(4096 // stride, 1))
                worst[name] = max(worst.get(name, 0.0), e)
        print(f"{k}: {x.shape} at {fft}/{hop}, kernel {kernel}, power {power}, margin {margin}: " +
              ", ".join(f"{n} {e:.2e}" for n, e in worst.items()) + " of the block peak")
        if k == OUT_EXEMPT:
            glob = max(float(np.max(np.abs(y[::stride].astype(np.float64) - gold[f"{k}{name}"]))) for name, y in (("_H", h), ("_P", p)))
            glob /= float(np.max(np.abs(x)))
            print(f"{k}: {glob:.2e} of the file's peak")
            assert max(worst.values()) <= OUT_EXEMPT_TOL and glob <= OUT_TOL, (k, worst, glob)
            continue
        worst_all = max(worst_all, max(worst.values()))
        assert max(worst.values()) <= OUT_TOL, (k, worst)
    print(f"separate: worst {worst_all:.3e} of the block peak over the capped settings")


def test_margin_one_components_sum_to_the_resynthesis(dev, gold, sigs):
    import torch
    from pyaudiorestoration_amd import _dev, fourier, hpss
    worst = 0.0
    for src, fft, hop, kernel in (("synth", 512, 128, (31, 31)), ("nr", 2048, 512, (17, 64)), ("nr", 16384, 4096, (31, 31)), ("rhythm2", 512, 128, (99, 99)),
                                   ("synth", 32768, 8192, (31, 31))):          # the four-step STFT and the scratch ISTFT around the kernel
        x = sigs[src][:, 0]
        h, p, r = hpss.separate(x, 44100, fft, hop, kernel)
        assert r is None and h.ndim == 1
        y = _dev.to_host(fourier.istft_dev(spectrum_dev(x, fft, hop, dev), hop, fourier.window_dev("blackmanharris", fft, dev), length=len(x), dev=dev))
        err = float(np.max(np.abs(h.astype(np.float64) + p - y))) / float(np.max(np.abs(y)))
        worst = max(worst, err)
        print(f"h + p against istft(stft(x)), {src} {fft}/{hop} {kernel}: {err:.3e} of the peak")
        assert err <= SUM_TOL, (src, fft, err)
    print(f"h + p: worst {worst:.3e} of the peak")
    assert SUM_TOL <= 1e-6


def test_stereo_equals_mono_channel_by_channel_and_residual(dev, gold, sigs):
    import torch
    from pyaudiorestoration_amd import _dev, hpss
    x = sigs["rhythm2"]
    for margin in (1.0, (2.0, 3.0)):
        h, p, r = hpss.separate(x, 44100, 512, 128, (31, 17), 2.0, margin)
        for c in range(2):
            h1, p1, r1 = hpss.separate(np.ascontiguousarray(x[:, c]), 44100, 512, 128, (31, 17), 2.0, margin)
            assert np.array_equal(h[:, c].view(np.uint32), h1.view(np.uint32)) and np.array_equal(p[:, c].view(np.uint32), p1.view(np.uint32))
            if r is not None:
                assert np.array_equal(r[:, c], r1) and np.array_equal(r[:, c], x[:, c] - (h[:, c] + p[:, c]))      # numpy's float32 residual
        assert (r is None) == (margin == 1.0)
    # one of two channels, a device tensor in, device tensors out
    t = _dev.to_dev(x, torch.float32, dev)
    h2, p2, r2 = hpss.separate(t, 44100, 512, 128, (31, 17), channels=[1])
    assert torch.is_tensor(h2) and h2.shape == (len(x), 1) and r2 is None
    h1, _, _ = hpss.separate(np.ascontiguousarray(x[:, 1]), 44100, 512, 128, (31, 17))
    assert np.array_equal(_dev.to_host(h2)[:, 0], h1)


def test_separate_file_and_cli_write_the_same_float_wavs(dev, gold, tmp_path):
    import shutil
    import struct
    from pyaudiorestoration_amd import hpss, io_ops
    a, b = tmp_path / "a", tmp_path / "b"
    for d in (a, b):
        d.mkdir()
        shutil.copy(os.path.join(GOLDEN, "nr_signal.wav"), d / "nr_signal.wav")
    paths = hpss.separate_file(str(a / "nr_signal.wav"), kernel=(31, 17), margin=(2.0, 3.0), device=dev)
    assert [os.path.basename(p) for p in paths] == ["nr_signal_H.wav", "nr_signal_P.wav", "nr_signal_R.wav"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "pyaudiorestoration_amd.cli", "hpss", "--kernel", "31,17", "--margin", "2,3", str(b / "nr_signal.wav")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    x, _, _ = io_ops.read_file(os.path.join(GOLDEN, "nr_signal.wav"))
    outs = []
    for p in paths:
        raw = open(p, "rb").read()
        assert raw == open(b / os.path.basename(p), "rb").read()
        tag, ch, sr, _, _, bits = struct.unpack("<HHIIHH", raw[20:36])
        assert (tag, ch, sr, bits) == (3, 1, 44100, 32)                 # IEEE float32 WAV
        y, _, _ = io_ops.read_file(p)
        assert y.shape == x.reshape(len(x), -1).shape
        outs.append(y)
    assert np.array_equal(outs[2], x.reshape(len(x), -1) - (outs[0] + outs[1]))
    only = hpss.separate_file(str(a / "nr_signal.wav"), device=dev)     # margin 1: no residual file is written
    assert [os.path.basename(p) for p in only] == ["nr_signal_H.wav", "nr_signal_P.wav"]
