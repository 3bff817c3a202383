"""Differential EQ without a GPU: difeq.eq_curve and difeq.export against what the reference's own MainWindow.plot / write
produced (tests/golden/difeq.npz, tools/gen_golden_difeq.py), bit for bit and byte for byte for every stored setting; the
fixture's own consistency; the argument contract of par_stft_mean_db_f32 and its scratch arithmetic."""
import ctypes
import os

import numpy as np
import pytest

import difeq_np as D


@pytest.fixture(scope="module")
def g():
    return D.fixture()


def settings():
    return [str(s) for s in D.fixture()["settings"]]


def _inputs(g, setting):
    names = [str(n) for n in g[f"{setting}_eqs"]]
    eqs = [np.array(D.pair_eq(g, n)) for n in names]
    freqs = np.arange(0, 8193) / 16384.0 * float(g[f"{names[-1]}_sr"][0])
    return freqs, eqs


def test_fixture_is_consistent(g):
    assert int(g["fft_size"]) == 16384 and int(g["hop"]) == 8192
    pairs = [str(p) for p in g["pairs"]]
    assert {"mono", "rhythm", "rates"} <= set(pairs)
    for p in pairs:
        eq, top = D.pair_eq(g, p), D.pair_top(g, p)
        assert eq.shape == top.shape == (2, 8193) and eq.dtype == np.float64 and np.all(np.isfinite(eq))
        assert g[f"{p}_src"].dtype == np.float32 and g[f"{p}_src"].shape == g[f"{p}_ref"].shape == g[f"{p}_eq"].shape
        assert np.all(top.mean(axis=1) >= 0.5) and np.allclose(top.mean(axis=1), g[f"{p}_share"])
        assert os.path.exists(os.path.join(D.GOLDEN, str(g[f"{p}_files"][0]))) and os.path.exists(os.path.join(D.GOLDEN, str(g[f"{p}_files"][1])))
        # the spectra that select the bins are the ones whose difference is stored
        assert np.max(np.abs((g[f"{p}_ref"].astype(np.float64) - g[f"{p}_src"]) - g[f"{p}_eq"])) < 1e-4
    assert list(g["rates_sr"]) == [44100, 48000] and list(g["mono_sr"]) == [44100, 44100]
    want = {"defaults", "keep_gain", "strength50", "highpass500", "rolloff15_18", "smoothing1", "smoothing200", "resolution20",
            "resolution2000", "two_eqs"}
    assert set(settings()) == want
    for s in settings():
        p = D.curve_params(g, s)
        k = len(range(0, 2000 - p["smoothing"] + 1, 2000 // p["resolution"]))
        assert g[f"{s}_freqs_av"].shape == (k,) and g[f"{s}_av"].shape == (2, k) and g[f"{s}_av"].dtype == np.float64
        assert g[f"{s}_txt"].shape == (3,) and all(str(t).count('" v') == k for t in g[f"{s}_txt"])
    assert len(g["defaults_freqs_av"]) == 196 and len(g["two_eqs_eqs"]) == 2
    assert D.curve_params(g, "keep_gain")["keep_gain"] is True and D.curve_params(g, "strength50")["strength"] == 50
    assert D.curve_params(g, "rolloff15_18")["rolloff_start"] == 15000 and D.curve_params(g, "highpass500")["highpass"] == 500


@pytest.mark.parametrize("setting", settings())
def test_eq_curve_and_export_equal_the_reference(g, tmp_path, setting):
    from pyaudiorestoration_amd import difeq
    freqs, eqs = _inputs(g, setting)
    with np.errstate(all="ignore"):
        freqs_av, av = difeq.eq_curve(freqs, eqs, **D.curve_params(g, setting))
    assert av.dtype == np.float64 and freqs_av.dtype == np.float64
    assert np.array_equal(freqs_av.view(np.uint64), g[f"{setting}_freqs_av"].view(np.uint64))
    assert np.array_equal(av.view(np.uint64), g[f"{setting}_av"].view(np.uint64))
    assert all(e.flags.writeable and np.array_equal(e, D.pair_eq(g, str(n))) for e, n in zip(eqs, g[f"{setting}_eqs"])), "eq_curve changed its input"
    paths = difeq.export(str(tmp_path / "eq"), freqs_av, av)
    assert [os.path.basename(p) for p in paths] == ["eq.txt", "eq_L.txt", "eq_R.txt"]
    for p, want in zip(paths, g[f"{setting}_txt"]):
        assert open(p, "rb").read() == str(want).encode()


def test_eq_curve_gain_and_defaults(g):
    from pyaudiorestoration_amd import difeq
    freqs, eqs = _inputs(g, "defaults")
    fa, av, gain = difeq.eq_curve(freqs, eqs, return_gain=True)
    assert np.array_equal(av, g["defaults_av"])
    fk, ak = difeq.eq_curve(freqs, eqs, keep_gain=True)
    assert np.array_equal(ak, g["keep_gain_av"])
    # the gain is the mean of the smoothed curve between the keys nearest 70 Hz and rolloff_end, before strength and fades
    i1, i2 = np.abs(fa - 70).argmin(), np.abs(fa - 22000).argmin()
    inner = slice(i1, min(i2, int(np.searchsorted(fa, 21000))))
    assert np.allclose((av - ak)[:, inner], gain, rtol=0, atol=1e-12)


def test_write_eq_txt_format(tmp_path):
    from pyaudiorestoration_amd import difeq
    p = str(tmp_path / "a.txt")
    difeq.write_eq_txt(p, np.array([20.5, 100.0]), np.array([-1.25, 3.0]))
    assert open(p).read() == ('FilterCurve: FilterLength="8191" InterpolateLin="0" InterpolationMethod="B-spline" '
                              'f0="20.5" v0="-1.25" f1="100.0" v1="3.0" ')


def test_process_refuses_before_touching_files_without_a_gpu(tmp_path):
    import torch
    from pyaudiorestoration_amd import cli, difeq
    with pytest.raises(SystemExit):
        cli.main(["difeq", "a.wav", "b.wav"])                      # --out is required
    with pytest.raises(SystemExit):
        cli.main(["difeq", "a.wav", "b.wav", "--out", "eq.txt", "--channels", "Mean"])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            difeq.process([(str(tmp_path / "missing.wav"), str(tmp_path / "missing2.wav"))], str(tmp_path / "eq.txt"))
        with pytest.raises(SystemExit, match="no CPU fallback"):
            cli.main(["difeq", "a.wav", "b.wav", "--out", str(tmp_path / "eq.txt")])


def test_mean_db_argument_errors_without_a_gpu():
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(64)
    ok = dict(x=p, n=1000, stride=2, n_ch=2, n_fft=512, hop=256, zp=1, win=p, mean=p, scratch=p, nbytes=1 << 30)

    def call(**kw):
        a = dict(ok, **kw)
        return L.par_stft_mean_db_f32(0, a["x"], a["n"], a["stride"], a["n_ch"], a["n_fft"], a["hop"], a["zp"], a["win"], a["mean"],
                                      a["scratch"], a["nbytes"], None)
    for name in ("x", "win", "mean", "scratch"):
        assert call(**{name: None}) == 1 and "null" in _lib.last_error(), name
    for kw in (dict(n=0), dict(hop=0), dict(zp=0), dict(n_fft=0), dict(n_ch=0), dict(n_ch=9, stride=9), dict(stride=1), dict(n_ch=3)):
        assert call(**kw) == 1 and "bad sizes" in _lib.last_error(), kw
    assert call(scratch=ctypes.c_void_p(68)) == 1 and "aligned" in _lib.last_error()
    for kw in (dict(n_fft=1000), dict(n_fft=8), dict(n_fft=32768), dict(n_fft=16384, zp=2), dict(n_fft=6, zp=4)):
        rc = call(**kw)
        assert rc == 3 and "power of two" in _lib.last_error(), kw
        with pytest.raises(_lib.ParUnsupported):
            _lib.check(rc)
    need = L.par_stft_mean_db_scratch_bytes(1000, 512, 256, 1, 2)
    assert need == D.scratch_bytes(1000, 512, 256, 1, 2) == 2 * 1 * 257 * 8
    assert call(nbytes=need - 1) == 4 and "scratch" in _lib.last_error()


def test_mean_db_scratch_bytes():
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    # unsupported sizes and bad arguments: 0
    for a in ((1000, 1000, 10, 1, 1), (1000, 8, 4, 1, 1), (1000, 32768, 64, 1, 1), (1000, 16384, 64, 2, 1), (0, 512, 256, 1, 1),
              (1000, 512, 0, 1, 1), (1000, 512, 256, 0, 1), (1000, 512, 256, 1, 0), (1000, 512, 256, 1, 9)):
        assert L.par_stft_mean_db_scratch_bytes(*a) == 0, a
    # monotone in the channel count, equal to the documented layout: one float64 row of bins per run of
    # R = max(16, ceil(n_frames / 512)) frames and channel
    for n, n_fft, hop, zp in ((1000, 512, 256, 1), (26_460_000, 16384, 8192, 1), (691_200_000, 16384, 8192, 1), (26_460_000, 4096, 256, 1),
                              (5000, 8, 1, 2), (100_000, 4096, 2048, 4)):
        sizes = [L.par_stft_mean_db_scratch_bytes(n, n_fft, hop, zp, c) for c in range(1, 9)]
        assert sizes == [D.scratch_bytes(n, n_fft, hop, zp, c) for c in range(1, 9)]
        assert all(b > a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
        nf = D.n_frames_of(n, n_fft, hop)
        assert sizes[0] <= 512 * (n_fft * zp // 2 + 1) * 8 and -(-nf // D.run_len(nf)) <= 512
    assert D.run_len(1) == D.run_len(8192) == 16 and D.run_len(8193) == 17 and D.run_len(84375) == 165
