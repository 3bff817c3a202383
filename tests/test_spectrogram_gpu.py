"""The spectrogram image through Python: golden magnitudes through a one-to-one picture, the route switch, a tone's row in the
three scales, a zoomed render against a one-to-one image reduced by numpy, and render_file / the CLI file to file."""
import json
import os
import shutil

import numpy as np
import pytest

import inputs
import spectrogram_np as SN
from test_hip_parity import TOL, relerr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def sp():
    from pyaudiorestoration_amd import spectrogram
    return spectrogram


def one_to_one(sp, n, sr, fft, hop, zp=1):
    """width = frames, one linear row per bin: f1 half a bin above the last bin puts bin H - r in row r"""
    frames = SN.stft_frames(n, fft, hop)
    bins = fft * zp // 2 + 1
    df = sr / (fft * zp)
    g = sp.geometry(n, sr, fft, hop, zp, frames, bins, f0=0.0, f1=(bins - 0.5) * df, scale="linear")
    assert np.array_equal(g.col_lo, np.arange(frames)) and np.array_equal(g.col_hi, np.arange(frames) + 1)
    assert np.array_equal(g.row_lo, np.arange(bins)[::-1]) and np.array_equal(g.row_hi, np.arange(bins)[::-1] + 1)
    return g


def as_spectrogram(peak):
    """(width, height) one-to-one image -> (bins, frames), bin 0 first"""
    return peak.T[::-1]


def test_one_to_one_image_holds_the_reference_magnitudes(sp, golden):
    g = golden["stft"]
    n, seed, n_fft, hop, zp = (int(v) for v in g["bh_cfg"])
    x = inputs.noise(n, seed)
    geo = one_to_one(sp, n, 44100.0, n_fft, hop, zp)
    want = np.abs(g["bh_S"].astype(np.complex128)) + 1e-7
    for fused in (True, False):
        m = as_spectrogram(sp.peak_image(x, 44100.0, geo, str(g["bh_win"]), fused=fused))
        assert m.shape == want.shape and relerr(m, want) < TOL, fused
    x = inputs.noise(4096, 0)
    geo = one_to_one(sp, 4096, 44100.0, 1024, 256)
    for fused in (True, False):
        m = as_spectrogram(sp.peak_image(x, 44100.0, geo, "blackmanharris", fused=fused))
        assert relerr(m, g["kat2_mag"]) < TOL, fused


@pytest.mark.parametrize("fused", [True, False])
def test_fused_flag_selects_the_route_and_both_give_the_same_bits(sp, monkeypatch, fused):
    x = np.stack([inputs.noise(30000, 5), inputs.noise(30000, 6)], axis=1)
    geo = sp.geometry(30000, 48000.0, 1024, 128, 1, 37, 50)
    taken = []
    monkeypatch.setattr(sp, "FUSED", fused)
    monkeypatch.setattr(sp, "_peak_fused_dev", lambda *a, _f=sp._peak_fused_dev: taken.append(True) or _f(*a))
    monkeypatch.setattr(sp, "_peak_composed_dev", lambda *a, _f=sp._peak_composed_dev: taken.append(False) or _f(*a))
    got = sp.peak_image(x, 48000.0, geo, channel=1)
    assert taken == [fused], "FUSED does not select the route"
    other = sp.peak_image(x, 48000.0, geo, channel=1, fused=not fused, max_bytes=40 * 513 * 4)      # (composed: chunks of 40 frames)
    assert taken == [fused, not fused]
    assert np.array_equal(got.view(np.uint32), other.view(np.uint32)) and got.min() > 0
    assert not np.array_equal(got, sp.peak_image(x, 48000.0, geo, channel=0))
    # above the fused sizes the flag changes nothing
    big = sp.geometry(30000, 48000.0, 32768, 8192, 1, 3, 9)
    del taken[:]
    sp.peak_image(x, 48000.0, big, channel=0)
    assert taken == [False]
    with pytest.raises(ValueError):
        sp.peak_image(x[:-1], 48000.0, geo)


@pytest.mark.parametrize("scale,f0", [("mel", None), ("linear", None), ("log", 40.0)])
def test_a_tone_lights_the_row_to_pixel_names(sp, scale, f0):
    sr, fft, hop = 32000.0, 512, 128                                         # 1 kHz is bin 16 exactly
    n = 20001                                                               # a cosine whose reflections at both ends continue it
    x = np.cos(2 * np.pi * 1000.0 * np.arange(n) / sr).astype(np.float32)
    for width, height, kw in ((50, 64, {}), (200, 300, dict(t0=-0.1, t1=0.9)), (9, 20, dict(t0=0.2, t1=0.5))):
        geo = sp.geometry(n, sr, fft, hop, 1, width, height, f0=f0, scale=scale, **kw)
        peak = sp.peak_image(x, sr, geo)
        lit = 0
        for c in range(width):
            if geo.col_hi[c] == geo.col_lo[c]:
                assert not peak[c].any()
                continue
            t = geo.col_times()[c] if geo.col_times()[c] >= 0 else 0.0
            px = geo.to_pixel(t, 1000.0)
            assert px is not None and geo.row_lo[px[1]] <= 16 < geo.row_hi[px[1]]
            assert peak[c, px[1]] == peak[c].max() and peak[c, px[1]] > 10 * np.median(peak[c])
            rows_with_it = np.flatnonzero((geo.row_lo <= 16) & (16 < geo.row_hi))
            assert np.argmax(peak[c]) == rows_with_it[0]                     # the brightest row (the first of them when magnified)
            lit += 1
        assert lit >= min(width, 9)


def test_zoomed_render_equals_the_region_of_a_one_to_one_image(sp):
    sr, fft, overlap = 22050.0, 256, 4
    n = 12000
    x = (inputs.noise(n, 9) * np.linspace(0.01, 1.0, n)).astype(np.float32)
    full = sp.peak_image(x, sr, one_to_one(sp, n, sr, fft, fft // overlap))  # (frames, bins), row r = bin H - r
    mag = as_spectrogram(full).T                                            # [frames][bins]
    kw = dict(width=23, height=31, fft_size=fft, overlap=overlap, t0=0.11, t1=0.37, f0=500.0, f1=7000.0, scale="mel")
    rgba, geo = sp.render(x, sr, vmin=-100.0, vmax=-10.0, cmap="gray", **kw)
    assert rgba.shape == (31, 23, 4) and rgba.dtype == np.uint8
    want_peak = SN.peak_np(mag, geo)
    assert np.array_equal(sp.peak_image(x, sr, geo).view(np.uint32), want_peak.view(np.uint32))
    want = SN.colorize_np(want_peak, -100.0, -10.0, sp.colormap("gray"))
    v = SN.colorize_t(want_peak, -100.0, -10.0).T
    near = np.abs(v - np.rint(v)) < 1e-6
    assert np.array_equal(rgba[~near], want[~near]) and np.abs(rgba.astype(int) - want.astype(int)).max() <= 1


def test_render_file_and_the_cli(sp, tmp_path, capsys):
    from pyaudiorestoration_amd import cli, io_ops
    src = str(tmp_path / "flutter.flac")
    shutil.copy(os.path.join(GOLDEN, "flutter.flac"), src)
    signal, sr, _ = io_ops.read_file(src)
    kw = dict(width=160, height=96, fft_size=1024, overlap=4, f0=100.0, f1=8000.0, scale="log")
    want, geo = sp.render(signal, sr, **kw)
    png, meta, geo2 = sp.render_file(src, **kw)
    assert png == str(tmp_path / "flutter_spec.png") and meta == str(tmp_path / "flutter_spec.json")
    assert np.array_equal(SN.png_decode(open(png, "rb").read()), want) and want[..., :3].any()
    back = sp.load_geometry(meta)
    assert back.args() == geo.args() == geo2.args() and np.array_equal(back.col_lo, geo.col_lo) and np.array_equal(back.row_lo, geo.row_lo)
    assert json.load(open(meta))["geometry"]["scale"] == "log"
    out = str(tmp_path / "cli.png")
    argv = ["spectrogram", src, "--size", "160,96", "--fft", "1024", "--overlap", "4", "--freq", "100,8000", "--scale", "log"]
    assert cli.main(argv + ["--out", out]) == 0
    assert np.array_equal(SN.png_decode(open(out, "rb").read()), want)
    assert sp.load_geometry(str(tmp_path / "cli.json")).args() == geo.args()
    capsys.readouterr()
    before = sorted(os.listdir(tmp_path))
    assert cli.main(argv + ["--at", "37,50"]) == 0
    t, f = (float(v) for v in capsys.readouterr().out.split())
    assert (t, f) == geo.to_time_freq(37, 50) and sorted(os.listdir(tmp_path)) == before
    # another range, colour limits and map: the arguments reach the picture
    assert cli.main(argv[:2] + ["--range", "0.5,1.5", "--size", "40,30", "--clim=-90,-20", "--cmap", "gray", "--channel", "0", "--out", out]) == 0
    small = SN.png_decode(open(out, "rb").read())
    want_small, _ = sp.render(signal, sr, width=40, height=30, t0=0.5, t1=1.5, vmin=-90, vmax=-20, cmap="gray")
    assert small.shape == (30, 40, 4) and np.array_equal(small, want_small)
