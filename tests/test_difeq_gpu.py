"""difeq.get_eq and the command line end to end on the GPU, against what the reference's own get_eq returned for the same files
(tests/golden/difeq.npz, tools/gen_golden_difeq.py).

Criterion (that of tests/test_expander_gpu.py's spectrum_flat tests, per spectrum): bins more than 60 dB under an averaged
spectrum's peak sit at the float32 rounding floor of any float32 STFT, the others agree with the reference within 2e-2 dB.  An EQ
is the difference of two such spectra: on the bins within 60 dB of the peak of BOTH, |ours - reference| <= 2 x 2e-2 dB.  Those
bins are at least half of all bins on every stored pair (checked when the fixture was generated, and again here)."""
import os

import numpy as np
import pytest

import difeq_np as D
import pan_np

pytestmark = pytest.mark.gpu
TOL_DB = 2 * 2e-2


@pytest.fixture(scope="module")
def g():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return D.fixture()


def pair_paths(g, pair, tmp_path):
    """the pair's files; the one whose stored rate differs from its header is written again with that rate"""
    from pyaudiorestoration_amd import io_ops
    paths = []
    for name, sr in zip(g[f"{pair}_files"], g[f"{pair}_sr"]):
        path = os.path.join(D.GOLDEN, str(name))
        sig, file_sr, _ = io_ops.read_file(path)
        if file_sr != int(sr):
            path = str(tmp_path / f"sr{int(sr)}.wav")
            io_ops.write_wav_float(path, sig, int(sr))
        paths.append(path)
    return paths


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("pair", ["mono", "rhythm", "rates"])
def test_get_eq_against_reference(g, tmp_path, monkeypatch, pair, fused):
    from pyaudiorestoration_amd import difeq
    src, ref = pair_paths(g, pair, tmp_path)
    monkeypatch.setattr(difeq, "FUSED", fused)
    taken = []
    monkeypatch.setattr(difeq.spectrum_flat, "mean_spectra_db_dev",
                        lambda *a, _f=difeq.spectrum_flat.mean_spectra_db_dev, **k: taken.append(k["fused"]) or _f(*a, **k))
    interps = []
    monkeypatch.setattr(difeq.np, "interp", lambda *a, _f=np.interp: interps.append(len(a[0])) or _f(*a))
    freqs, eq = difeq.get_eq(src, ref, str(g[f"{pair}_mode"]))
    assert taken == [fused, fused], "FUSED does not select the path"
    want, top = D.pair_eq(g, pair), D.pair_top(g, pair)
    sr_src, sr_ref = (int(v) for v in g[f"{pair}_sr"])
    assert eq.shape == want.shape == (2, 8193) and eq.dtype == np.float64 and freqs.shape == (8193,) and freqs[-1] == sr_src / 2
    assert interps == ([8193, 8193] if sr_src != sr_ref else []), "np.interp is for pairs whose rates differ, once per spectrum"
    assert np.all(top.mean(axis=1) >= 0.5)
    err = np.abs(eq - want)
    print(f"\n{pair} fused={fused}: max |ours - reference| {err.max():.3e} dB, within 60 dB of both peaks {err[top].max():.3e} "
          f"({top.mean():.0%} of the bins)", end="")
    assert err[top].max() <= TOL_DB
    assert np.array_equal(eq[0], eq[1])                      # mono files: the only spectrum is used twice


def test_mono_fallback_and_right_channel_of_a_mono_file(g):
    from pyaudiorestoration_amd import difeq
    path = os.path.join(D.GOLDEN, "nr_noise.wav")
    both, sr = difeq.spectra_stereo(path, channel_mode="L+R")
    left, _ = difeq.spectra_stereo(path, channel_mode="L")
    mean, _ = difeq.spectra_stereo(path, channel_mode="Mean")
    assert sr == 44100 and len(both) == len(left) == len(mean) == 2
    assert all(np.array_equal(both[0], s) for s in (both[1], left[0], left[1], mean[0], mean[1]))
    with pytest.raises(ValueError, match="nr_noise.wav"):
        difeq.spectra_stereo(path, channel_mode="R")
    with pytest.raises(ValueError, match="nr_noise_eq4.wav"):
        difeq.get_eq(os.path.join(D.GOLDEN, "nr_noise_eq4.wav"), path, "R")


def test_stereo_file_channels(g, tmp_path):
    """two different channels: L+R in one launch; R alone is the second row bit for bit; both paths agree far inside the criterion"""
    from pyaudiorestoration_amd import difeq, io_ops
    tape = pan_np.stereo_tape()
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    io_ops.write_wav_float(a, tape, pan_np.SR)
    io_ops.write_wav_float(b, (tape * np.float32(0.5))[:, ::-1].copy(), pan_np.SR)
    _, eq = difeq.get_eq(a, b, "L+R", fused=True)
    _, eq_r = difeq.get_eq(a, b, "R", fused=True)
    _, eq_l = difeq.get_eq(a, b, "L", fused=True)
    _, eq_c = difeq.get_eq(a, b, "L+R", fused=False)
    assert eq.shape == (2, 8193) and not np.array_equal(eq[0], eq[1])
    assert np.array_equal(eq_r[0], eq[1]) and np.array_equal(eq_r[1], eq[1]) and np.array_equal(eq_l[0], eq[0]) and np.array_equal(eq_l[1], eq[0])
    assert np.max(np.abs(eq - eq_c)) <= 1e-9


def test_cli_end_to_end(g, tmp_path):
    from pyaudiorestoration_amd import cli, difeq
    src, ref = pair_paths(g, "mono", tmp_path)
    out = tmp_path / "eq.txt"
    assert cli.main(["difeq", src, ref, "--out", str(out)]) == 0
    keys = len(g["defaults_freqs_av"])
    texts = []
    for name in ("eq.txt", "eq_L.txt", "eq_R.txt"):
        text = (tmp_path / name).read_text()
        assert text.startswith(difeq.HEADER) and text.count('" v') == keys and f'f{keys - 1}="' in text and f'f{keys}="' not in text
        texts.append(text)
    assert texts[1] == texts[2] == texts[0]                  # a mono pair: both channels, and so their mean, are one curve
    # the keys' frequencies are the reference's to the bit (they do not depend on the spectra)
    assert texts[0].split(" v0=")[0] == str(g["defaults_txt"][0]).split(" v0=")[0]
    assert cli.main(["difeq", src, ref, src, ref, "--out", str(tmp_path / "two.eq.txt"), "--resolution", "20", "--keep-gain"]) == 0
    assert (tmp_path / "two.eq.txt").read_text().count('" v') == len(g["resolution20_freqs_av"]) and (tmp_path / "two.eq_L.txt").exists()
