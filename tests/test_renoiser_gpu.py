"""GPU checks of the renoiser port (renoiser_gui.Canvas): the standalone gate against numpy on K_stft's own spectrum (bit for
bit), the fused kernel against the composed device path, and both against the reference's own outputs (tests/golden/renoiser.npz,
written by tools/gen_golden_renoiser.py).  Measured errors are printed (pytest -s) for NOTES.md."""
import os
import subprocess
import sys

import numpy as np
import pytest

import renoiser_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PROFILE_DB = 2e-3          # our noise-file profiles against the reference's (dB; measured 1.2e-4)
SELECT_DB = 1e-2           # the selection profile, a mean of magnitudes down to the FFT's rounding floor (measured 3.3e-3; NOTES.md)
OUT_BLOCK = 1e-5           # output per 4096-sample block where the masks agree (relative to the block's peak)
FUSED_TOL = 1e-6           # fused against composed (relative to the output's peak)


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return 0


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "renoiser.npz"))


@pytest.fixture(scope="module")
def wavs():
    from pyaudiorestoration_amd import io_ops
    sig, sr, _ = io_ops.read_file(os.path.join(GOLDEN, "nr_signal.wav"))
    noise, _, _ = io_ops.read_file(os.path.join(GOLDEN, "nr_noise.wav"))
    return (sig if sig.ndim == 2 else sig[:, None]), (noise if noise.ndim == 2 else noise[:, None]), sr


def block_relerr(a, b, block=4096, floor_db=-80, blocks=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    floor = np.max(np.abs(b)) * 10 ** (floor_db / 20)
    worst = 0.0
    for i, s in enumerate(range(0, len(b), block)):
        if blocks is not None and not blocks[i]:
            continue
        ref = max(float(np.max(np.abs(b[s:s + block]))), floor)
        worst = max(worst, float(np.max(np.abs(a[s:s + block] - b[s:s + block]))) / ref)
    return worst


def spectrum_dev(x, fft, hop, dev):
    """K_stft mode 0 of fix_length(x, n + fft/2): (frames, bins) complex64 device tensor"""
    import torch
    from pyaudiorestoration_amd import _dev, fourier
    xp = np.zeros(len(x) + fft // 2, np.float32)
    xp[:len(x)] = x
    spec = fourier.stft_dev(_dev.to_dev(xp, torch.float32, dev), fft, hop, fourier.window_dev("blackmanharris", fft, dev), 1, 0, dev=dev)
    return spec.T


def test_gate_spectrum_is_bit_identical_to_numpy_on_k_stft_spectrum(dev, wavs):
    import torch
    from pyaudiorestoration_amd import _dev, _lib, renoiser
    sig = wavs[0][:, 0]
    rng = np.random.default_rng(7)
    L = _lib.lib()
    for fft, hop, gain in ((64, 16, 12.0), (512, 128, -20.0), (2048, 512, 12.0), (8192, 2048, 6.0), (16384, 4096, 12.0),
                           (32768, 8192, -9.0)):
        fm = spectrum_dev(sig, fft, hop, dev)
        S = _dev.to_host(fm).copy()
        db = renoiser_np.db32(np.abs(S) + np.float32(1e-7)).astype(np.float64)
        final = np.median(db, axis=0) + rng.uniform(-3, 3, S.shape[1])
        final[::97] = db[len(S) // 2, ::97]                       # exact ties: a bin on its threshold is gated
        final[5] = np.nan
        cut = _dev.to_dev(renoiser.gate_cutoffs(final), torch.float32, dev)
        _lib.check(L.par_gate_spectrum_f32(dev, _dev.ptr(fm), fm.shape[0], fm.shape[1], 0, _dev.ptr(cut), float(renoiser.low_factor(gain)),
                                           _dev.stream_ptr(dev)))
        got = _dev.to_host(fm)
        want = renoiser_np.gate(S, final, gain)
        share = float(np.mean(renoiser_np.passes(S, final)))
        print(f"gate {fft}/{hop}: {S.shape} bins, {share:.3f} pass, bit-identical {np.array_equal(got.view(np.uint32), want.view(np.uint32))}")
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (fft, hop)


def _final_for(x, fft, hop, dev):
    """a threshold profile under which about half the bins pass: the per-bin median dB of x's spectrum"""
    from pyaudiorestoration_amd import _dev
    S = _dev.to_host(spectrum_dev(x, fft, hop, dev))
    return np.median(renoiser_np.db32(np.abs(S) + np.float32(1e-7)).astype(np.float64), axis=0)


def test_fused_equals_composed(dev, wavs):
    import torch
    from pyaudiorestoration_amd import _dev, renoiser
    rng = np.random.default_rng(108)
    base = wavs[0][:, 0]
    worst = 0.0
    cases = 0
    for fft in (64, 128, 256, 512, 1024, 2048, 4096, 8192):
        for overlap in (1, 4, 16, 32):
            hop = fft // overlap
            final = _final_for(base[:20000], fft, hop, dev)
            for kind in ("mono", "stereo", "one_of_two", "short"):
                n = {"mono": 20001, "stereo": 17777, "one_of_two": 12345, "short": max(1, fft // 2 - 3)}[kind]
                off = int(rng.integers(0, len(base) - n))
                x = base[off:off + n]
                if kind in ("stereo", "one_of_two"):
                    x2 = np.stack([x, np.roll(x, 333) * np.float32(0.7)], axis=1)
                else:
                    x2 = x[:, None] + rng.standard_normal((n, 1)).astype(np.float32) * np.float32(1e-3)
                chans = [0] if kind == "one_of_two" else None
                sig_t = _dev.to_dev(np.ascontiguousarray(x2), torch.float32, dev)
                a = _dev.to_host(renoiser.renoise_dev(sig_t, final, 12.0, fft, hop, chans, dev, fused=True))
                b = _dev.to_host(renoiser.renoise_dev(sig_t, final, 12.0, fft, hop, chans, dev, fused=False))
                assert a.shape == b.shape == (n, 1 if chans else x2.shape[1])
                assert np.isfinite(a).all()
                peak = max(float(np.max(np.abs(b))), 1e-30)
                err = float(np.max(np.abs(a.astype(np.float64) - b))) / peak
                worst = max(worst, err)
                cases += 1
                assert err <= FUSED_TOL, (fft, hop, kind, err)
    print(f"fused vs composed: {cases} cases, largest difference {worst:.3e} of the peak")


def _setting(gold, k):
    fft, hop, gain, overhead, stride = gold[f"{k}_params"]
    return int(fft), int(hop), float(gain), float(overhead), int(stride)


def test_against_the_reference_fixtures(dev, gold, wavs):
    import torch
    from pyaudiorestoration_amd import _dev, renoiser
    sig, noise, sr = wavs
    for k in gold["settings"]:
        fft, hop, gain, overhead, stride = _setting(gold, k)
        signal = np.concatenate([sig, np.roll(sig, int(gold["stereo_shift"]), axis=0)], axis=1) if k == "stereo" else sig
        n = len(signal)
        if k == "noprofile":
            prof = renoiser.default_profile(sr, fft)
            assert np.array_equal(prof, gold[f"{k}_noise_profile"])
        elif k == "select":
            t0, t1 = gold["selection"]
            prof = renoiser.noise_profile_from_selection(signal, sr, t0, t1, fft, hop, 0, dev)
        else:
            prof = renoiser.noise_profile(noise, sr, sr, fft, hop, dev)
        perr = float(np.max(np.abs(prof.astype(np.float64) - gold[f"{k}_noise_profile"])))
        assert perr <= (SELECT_DB if k == "select" else PROFILE_DB), (k, perr)
        final = renoiser.final_profile(prof, sr, fft, gain, overhead, gold[f"{k}_curve"].tolist())
        y = renoiser.renoise(signal, sr, final, gain, fft, hop)
        assert y.shape == (n, signal.shape[1]) and y.dtype == np.float32 and np.isfinite(y).all()
        near = gold[f"{k}_near"]
        frames = int(gold[f"{k}_frames"])
        bins = fft // 2 + 1
        worst, flips = 0.0, 0
        for c in range(signal.shape[1]):
            S = _dev.to_host(spectrum_dev(signal[:, c], fft, hop, dev))
            cut = renoiser.gate_cutoffs(final)
            ours = (np.abs(S) + np.float32(1e-7)) >= cut[None, :]
            ref = np.unpackbits(gold[f"{k}_mask"][c])[:frames * bins].reshape(frames, bins).astype(bool)
            exempt = np.zeros_like(ref)
            mine = near[near[:, 0] == c]
            exempt[mine[:, 1], mine[:, 2]] = True
            bad = (ours != ref) & ~exempt
            assert not bad.any(), (k, c, np.argwhere(bad)[:5])
            dis = np.argwhere(ours != ref)
            flips += len(dis)
            # output blocks no disagreeing bin can reach
            ok = np.ones(-(-n // 4096), bool)
            for lo, hi in renoiser_np.reach(dis[:, 0], hop, fft, n):
                ok[lo // 4096:(hi - 1) // 4096 + 1] = False
            yc = y[::stride, c]
            blocks = ok[(np.arange(len(yc)) * stride) // 4096]
            # strided samples: compare block by block in the strided index space (4096 // stride samples per block)
            err = block_relerr(yc, gold[f"{k}_y"][:, c], 4096 // stride, blocks=blocks[::4096 // stride])
            worst = max(worst, err)
        print(f"{k}: profile {perr:.2e} dB, {len(near)} near-threshold bins, {flips} disagreeing bins, output {worst:.2e} of the block peak")
        assert worst <= OUT_BLOCK, (k, worst)


def test_renoise_file_and_cli_write_the_same_bytes(dev, gold, tmp_path):
    import shutil
    from pyaudiorestoration_amd import io_ops, renoiser
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    for d in (a, b):
        shutil.copy(os.path.join(GOLDEN, "nr_signal.wav"), d / "nr_signal.wav")
    path = renoiser.renoise_file(str(a / "nr_signal.wav"), noise_path=os.path.join(GOLDEN, "nr_noise.wav"), device=dev)
    assert os.path.basename(path) == "nr_signal fft=2048.wav" and os.path.exists(path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "pyaudiorestoration_amd.cli", "renoise", "--noise", os.path.join(GOLDEN, "nr_noise.wav"),
                        str(b / "nr_signal.wav")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    other = b / "nr_signal fft=2048.wav"
    assert open(path, "rb").read() == open(other, "rb").read()
    y, sr, ch = io_ops.read_file(path)
    y = y if y.ndim == 2 else y[:, None]
    assert (sr, ch, len(y)) == (44100, 1, 40982)
    assert block_relerr(y[:, 0], gold["default_y"][:, 0]) <= OUT_BLOCK * 10     # the default setting's 2 near bins included


def test_full_size_stereo_fused_against_composed(dev):
    import torch
    from pyaudiorestoration_amd import _dev, renoiser
    sr, n = 44100, 44100 * 600
    g = torch.Generator(device=f"cuda:{dev}").manual_seed(5)
    t = torch.arange(n, device=f"cuda:{dev}", dtype=torch.float64) / sr
    tone = (0.3 * torch.sin(2 * np.pi * 440.0 * t) * (1 + 0.5 * torch.sin(2 * np.pi * 0.05 * t))).to(torch.float32)
    x = torch.stack([tone, torch.roll(tone, 12345)], dim=1) + 0.01 * torch.randn((n, 2), generator=g, device=f"cuda:{dev}")
    x = x.contiguous()
    final = _final_for(_dev.to_host(x[:200000, 0]), 2048, 512, dev)
    a = renoiser.renoise_dev(x, final, 12.0, 2048, 512, None, dev, fused=True)
    b = renoiser.renoise_dev(x, final, 12.0, 2048, 512, None, dev, fused=False)
    assert a.shape == (n, 2)
    assert not bool(torch.isnan(a).any())
    peak = float(b.abs().max())
    worst = 0.0
    for s in range(0, n, 1 << 22):
        worst = max(worst, float((a[s:s + (1 << 22)].double() - b[s:s + (1 << 22)].double()).abs().max()) / peak)
    print(f"10-min stereo 2048/512: fused vs composed {worst:.3e} of the peak")
    assert worst <= FUSED_TOL
