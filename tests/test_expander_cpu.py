"""CPU checks of the Spectral Expander / spectrum_flat port: the reference's bin and smoothing arithmetic, the channel-mode
mapping, the fixtures, and the `expand` subcommand's parser.  No GPU needed."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_freq2bin_follows_the_reference_rule():
    from pyaudiorestoration_amd import expander
    nb = 257
    # expander_gui.py:128-129: max(1, min(num_bins - 3, int(round(f * fft_size / sr))))
    assert expander.freq2bin(13000, nb, 512, 44100) == 151
    assert expander.freq2bin(17000, nb, 512, 44100) == 197
    assert expander.freq2bin(0, nb, 512, 44100) == 1                 # clamped below
    assert expander.freq2bin(22050, nb, 512, 44100) == nb - 3        # clamped above
    assert expander.freq2bin(22000, nb, 512, 192000) == 59


def test_smoothing_window_is_odd_frames():
    from pyaudiorestoration_amd import expander
    assert expander.smoothing_size(.11, 44100, 64) == 75              # int(75.796...) = 75, already odd
    assert expander.smoothing_size(.11, 48000, 64) == 83              # 82 -> 83
    assert expander.smoothing_size(5, 192000, 64) == 15001            # the GUI's longest window at 192 kHz
    assert expander.smoothing_size(.001, 8000, 64) == 1               # 0 -> 1


def test_channel_modes():
    from pyaudiorestoration_amd import expander, spectrum_flat
    assert spectrum_flat.channel_map == {"L": (0,), "R": (1,), "L+R": (0, 1), "Mean": (0, 1)}
    assert expander.analysed_channels("L+R", 2) == [0, 1]
    assert expander.analysed_channels("L+R", 1) == [0]               # mono fallback
    assert expander.analysed_channels("Mean", 1) == [0]
    assert expander.analysed_channels("R", 1) == []                  # spectrum_from_audio_stereo then fails on spectra[0]
    assert expander.analysed_channels("R", 2) == [1]


def test_reference_signatures_are_kept():
    import inspect
    from pyaudiorestoration_amd import spectrum_flat
    for name in ("spectra_from_audio", "spectrum_from_audio", "spectrum_from_audio_stereo"):
        sig = inspect.signature(getattr(spectrum_flat, name))
        assert list(sig.parameters) == ["filename", "fft_size", "hop", "channel_mode", "temporal_mean"]
        assert [p.default for p in sig.parameters.values()][1:] == [4096, 256, "L", True]


@pytest.mark.parametrize("name", ["expander.npz", "spectrum_flat.npz"])
def test_fixtures_present_and_small(name):
    path = os.path.join(GOLDEN, name)
    assert os.path.getsize(path) <= 1 << 20
    z = np.load(path)
    assert "backend" in z.files and len(z["backend"]) == 1


def test_fixture_material_crosses_both_clip_bounds():
    import expander_inputs
    z = np.load(os.path.join(GOLDEN, "expander.npz"))
    tape = expander_inputs.stereo_tape()
    assert float(np.sum(tape, dtype=np.float64)) == float(z["tape_sum"])          # the seeded input is what the fixture saw
    c = z["LpR_curves"]
    assert c.min() < -120 and c.max() > -85


def test_cli_parses_expand_with_defaults(monkeypatch):
    from pyaudiorestoration_amd import cli
    seen = {}

    class Stop(Exception):
        pass

    def fake_basic_config(**kw):
        raise Stop
    import argparse
    orig = argparse.ArgumentParser.parse_args

    def grab(self, argv=None, namespace=None):
        ns = orig(self, argv, namespace)
        seen["ns"] = ns
        return ns
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", grab)
    monkeypatch.setattr(cli.logging, "basicConfig", fake_basic_config)
    with pytest.raises(Stop):
        cli.main(["expand", "tape.wav"])
    ns = seen["ns"]
    assert ns.cmd == "expand" and ns.files == ["tape.wav"]
    assert ns.channels == "L+R" and ns.band == [13000.0, 17000.0] and ns.clip == [-120.0, -85.0]
    assert ns.smoothing == .11 and ns.transition == 0 and ns.order == 1
    assert ns.fft_size == 512 and ns.hop == 64 and ns.suffix == "_decompressed" and ns.gpus == 0
    with pytest.raises(Stop):
        cli.main(["expand", "--channels", "Mean", "--band", "12000,16000", "--clip=-110,-80", "--transition", "4000", "--order", "2",
                  "a.flac", "b.wav"])
    ns = seen["ns"]
    assert ns.channels == "Mean" and ns.band == [12000.0, 16000.0] and ns.clip == [-110.0, -80.0] and ns.files == ["a.flac", "b.wav"]
    with pytest.raises(SystemExit):
        cli.main(["expand", "--channels", "X", "a.wav"])
