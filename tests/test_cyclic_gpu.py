"""Cyclic wow end to end on the GPU: cyclic_wow.analyse on tests/golden/cyclic_pilot.wav, fused and composed, against what the
reference's own script computed from that file (tests/golden/cyclic.npz).

The cycle length, and with it the cycle duration and the rpm, must be the reference's exactly.  The track and the fold carry the
float32 transform's noise through a parabola; their margin is not chosen here: the composed path at the parent's kernels (K_stft
mode 1, par_track_peak_f64) was measured against the golden on the MI355X, and the fused path gets four times that
(tests/cyclic_np.py: COMPOSED_DEV_*, MARGIN_*).  Figures printed with -s; NOTES.md "Cyclic wow" records them."""
import os

import numpy as np
import pytest

import cyclic_np as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PILOT = os.path.join(ROOT, "tests", "golden", "cyclic_pilot.wav")


@pytest.fixture(scope="module")
def runs(golden):
    """-> (golden, {fused: CyclicWow}) -- analysed once, shared, never written to"""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    from pyaudiorestoration_amd import cyclic_wow as W
    g = {k: v for k, v in golden["cyclic"].items()}
    return g, {fused: W.analyse(PILOT, rpm=float(g["rpm"]), pilot_hz=float(g["pilot_hz"]), fused=fused) for fused in (True, False)}


def deviations(res, g):
    return float(np.max(np.abs(res.freqs - g["freqs"]))), float(np.max(np.abs(res.avg - g["avg"])))


def test_cycle_length_duration_and_rpm_are_the_references(runs):
    g, by = runs
    for fused, res in by.items():
        assert res.frames_per_rotation == int(g["best"][0]) == 227, fused
        assert res.cycle_duration == float(g["cycle_duration"]) and res.rpm_measured == float(g["rpm_measured"])
        assert np.array_equal(res.results[:, 0], g["results"][:, 0]) and res.results.shape == (44, 2)
        assert np.array_equal(res.times, g["times"]) and len(res.freqs) == 2067
        assert int(np.argmax(res.results[:, 1])) == int(np.argmax(g["results"][:, 1]))


def test_track_and_fold_within_the_measured_margin(runs):
    """composed: the yardstick, within its own recorded deviation; fused: within four times the yardstick"""
    g, by = runs
    df_c, da_c = deviations(by[False], g)
    df_f, da_f = deviations(by[True], g)
    print(f"\ncomposed: max |freqs - ref| {df_c:.3e} Hz, max |avg - ref| {da_c:.3e} oct; fused: {df_f:.3e} Hz, {da_f:.3e} oct; "
          f"|delta - ref| fused {abs(by[True].delta - g['best'][1]):.3e} composed {abs(by[False].delta - g['best'][1]):.3e}", end="")
    assert df_c <= C.COMPOSED_DEV_FREQS and da_c <= C.COMPOSED_DEV_AVG, (df_c, da_c)
    assert df_f <= C.MARGIN_FREQS and da_f <= C.MARGIN_AVG, (df_f, da_f)
    for res in by.values():
        assert abs(res.delta - float(g["best"][1])) <= 2 * C.MARGIN_AVG
        assert np.max(np.abs(res.results[:, 1] - g["results"][:, 1])) <= 2 * C.MARGIN_AVG


def test_fused_and_composed_tracks_are_bit_identical_without_db(runs):
    from pyaudiorestoration_amd import cyclic_wow as W, io_ops
    g, _ = runs
    signal, sr, _ = io_ops.read_file(PILOT)
    trail = [(0.0, 700.0), (len(signal) / sr, 700.0)]
    a = W.pilot_track(signal, sr, list(trail), db=False, fused=True)
    b = W.pilot_track(signal, sr, list(trail), db=False, fused=False)
    c = W.pilot_track(signal, sr, list(trail), db=False, fused=False, chunk_bytes=300 * 8193 * 4)      # seven chunks
    assert (a[2], a[3]) == (b[2], b[3]) == (0, 2067) and np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and np.array_equal(a[1].view(np.uint64), c[1].view(np.uint64))
    # "Peak Track" likewise, on a span inside the file; a device tensor and a strided channel go in as they are
    import torch
    stereo = torch.from_numpy(np.stack((np.full(len(signal), np.nan, dtype=np.float32), signal[:, 0]), axis=-1)).cuda()
    span = [(1.0, 700.0), (9.0, 700.0)]
    d = W.pilot_track(stereo, sr, list(span), channel=1, db=False, mode="Peak Track", fused=True)
    e = W.pilot_track(signal[:, 0], sr, list(span), db=False, mode="Peak Track", fused=False)
    assert d[2] == e[2] == int(1.0 * sr / 128) and np.array_equal(d[1].view(np.uint64), e[1].view(np.uint64))


def test_speed_curve_flattens_the_pilot(runs, tmp_path):
    """speed_curve -> resampling.run removes the measured cycle: the re-analysed depth drops (ratio printed, only < 1 asserted)"""
    from pyaudiorestoration_amd import cyclic_wow as W, io_ops, resampling
    g, by = runs
    res = by[True]
    signal, sr, _ = io_ops.read_file(PILOT)
    path = str(tmp_path / "pilot.wav")
    resampling.run((path,), signal_data=((signal, sr),), speed_curve=W.speed_curve(res, sr, 128), resampling_mode="Sinc", sinc_quality=32)
    again = W.analyse(str(tmp_path / "pilot_res.wav"), rpm=float(g["rpm"]), pilot_hz=float(g["pilot_hz"]))
    print(f"\ndepth {res.delta:.6f} -> {again.delta:.6f} octaves (ratio {again.delta / res.delta:.4f})", end="")
    assert again.delta < res.delta
