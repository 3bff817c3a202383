"""Fixture of the tape-sync tool's azimuth mode, computed by the REFERENCE's own code (build container only).

    python tools/gen_golden_azimuth.py --ref /path/to/pyaudiorestoration

The reference's modules are imported through oracle/ref_gui.py's import hook (stand-ins for the absent PyQt5 / vispy packages).  On
a stand-in canvas whose two spectra carry the reference's own Spectrum.get_signal / get_signal_around / get_times_freqs over
tests/golden/rhythm.flac and rhythm+5percent.flac (read with this project's FLAC reader), with the two LagSample markers of
tests/golden/rhythm.tapesync and the reference's LagLine, it runs unchanged

  pytapesynch_gui.Canvas.on_mouse_release, `Alt` branch (:210-238), through Canvas.correlate_sources (:108-133), match_speed off
  markers.AzimuthLine.update_reject (util/markers.py:542-552)   (called by that branch)
  markers.LagLine.update (:779-794) over the two markers plus the new line, unfiltered and with a 0 .. 2 Hz band

and stores only the inputs' parameters and arrays the reference computed: tests/golden/azimuth.npz

  sr, hop, smoothing, duration, len_ref, len_src, t0, t1, lower, upper, dur, overlap, reject, bands
  lag_curve0                        LagLine.data before the line exists (the curve the branch samples): its rows around the selection,
                                    which are all np.interp reads
  sample_times, sample_lags         np.arange / np.interp of the branch
  lags_raw, lags, corrs             AzimuthLine.lags_raw, .lags after update_reject, .corrs
  ref_geom, src_geom                (start, length, pad_l, pad_r) of every Spectrum.get_signal call, recorded around the method
  curve_len, curve_rows             LagLine.data with the line has curve_len rows; kept are the rows curve_rows: every row from 20
                                    before the line to 20 behind it, every 97th row, the last five
  curve_unfiltered, curve_filtered  those rows of LagLine.data (filtered: scipy's sosfiltfilt, as the reference runs it)

The installed numpy no longer has the np.NaN alias update_reject uses: the tool defines it as np.nan before the call.
Deterministic: running it twice writes identical files."""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gen_golden_expander import save  # noqa: E402
from oracle import ref_gui  # noqa: E402

DUR, OVERLAP, REJECT = 0.05, 4, 0.1
BOX = ((10.0, 300.0), (10.5, 5000.0))                  # Alt-drag: 0.5 s where both files have signal
BANDS = (0, 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (pyaudiorestoration)")
    a = ap.parse_args()
    _, _, markers, _ = ref_gui.import_reference_gui(a.ref)
    import pytapesynch_gui as T
    from util import spectrum as ref_spectrum
    from pyaudiorestoration_amd import io_ops
    if not hasattr(np, "NaN"):
        np.NaN = np.nan
    golden = os.path.join(ROOT, "tests", "golden")
    cfg = json.load(open(os.path.join(golden, "rhythm.tapesync")))
    ref_sig, sr, _ = io_ops.read_file(os.path.join(golden, "rhythm.flac"))
    src_sig, sr2, _ = io_ops.read_file(os.path.join(golden, "rhythm+5percent.flac"))
    assert sr == sr2
    hop = cfg["fft_size"] // cfg["fft_overlap"]

    c = ref_gui.fake_canvas(sr, cfg["fft_size"], hop, duration=len(src_sig) / sr)
    type_c = type("Canvas", (ref_gui.NS,), {})
    c.__class__ = type_c
    type_c.lags = property(lambda self: [m for m in self.markers if isinstance(m, markers.LagSample)])
    type_c.azimuths = property(lambda self: [m for m in self.markers if isinstance(m, markers.AzimuthLine)])
    geoms = [[], []]

    def spectrum_of(signal, which):
        s = ref_gui.NS(signal=signal, sr=sr, selected_channel=0, mel_transform=ref_gui._Anything(), offset=0.0)
        get_signal = ref_spectrum.Spectrum.get_signal

        def recording(self, t0, t1):                   # the method itself, and what it was asked: nothing of it is restated
            out = get_signal(self, t0, t1)
            s0, s1, n = int(t0 * self.sr), int(t1 * self.sr), len(self.signal)
            start, stop, _ = slice(s0, s1).indices(n)
            pad_l, pad_r = (abs(s0) if s0 < 0 else 0), (s1 - n if s1 > n else 0)
            assert len(out) == pad_l + max(0, stop - start) + pad_r
            assert np.array_equal(out[pad_l:len(out) - pad_r], self.signal[start:max(start, stop), 0])
            geoms[which].append((start, max(0, stop - start), pad_l, pad_r))
            return out
        s.get_signal = types.MethodType(recording, s)
        ref_gui._bind(s, ref_spectrum.Spectrum, "get_signal_around", "get_times_freqs")
        return s
    c.spectra = [spectrum_of(ref_sig, 0), spectrum_of(src_sig, 1)]
    c.filenames = ["rhythm.flac", "rhythm+5percent.flac"]
    c.parent = ref_gui.NS(props=ref_gui.NS(alignment_widget=ref_gui.NS(
        win_s=ref_gui.NS(value=lambda: DUR), overlap_s=ref_gui.NS(value=lambda: OVERLAP), reject_s=ref_gui.NS(value=lambda: REJECT),
        match_speed=False, ignore_phase=False)))
    pushed = []
    c.props.undo_stack = ref_gui.NS(push=lambda action: pushed.extend(action.traces))
    c.px_to_spectrum = lambda click: click
    ref_gui._bind(c, T.Canvas, "correlate_sources")
    for m in cfg["markers"]:
        markers.LagSample.from_cfg(c, *m).initialize()
    c.lag_line = markers.LagLine(c)
    c.lag_line.smoothing = cfg["smoothing"]
    c.lag_line.update()
    lag_curve0 = np.array(c.lag_line.data)

    event = ref_gui.NS(trail=lambda: [BOX[0]], pos=BOX[1], button=1, modifiers=("Alt",))
    stdout, sys.stdout = sys.stdout, open(os.devnull, "w")          # correlate_sources prints every delay
    try:
        T.Canvas.on_mouse_release(c, event)
    finally:
        sys.stdout = stdout
    assert len(pushed) == 1 and isinstance(pushed[0], markers.AzimuthLine)
    line = pushed[0]
    W = len(line.times)
    assert len(geoms[0]) == len(geoms[1]) == W and W >= 30
    t0, t1, lower, upper = c.spectra[0].get_times_freqs(*BOX)
    sample_lags = np.interp(line.times, lag_curve0[:, 0], lag_curve0[:, 1])
    line.initialize()                                                # AddAction.redo: the line joins the canvas' markers
    c.lag_line.update()
    curve_unfiltered = np.array(c.lag_line.data)
    c.lag_line.bands = BANDS
    c.lag_line.update()
    curve_filtered = np.array(c.lag_line.data)
    assert curve_unfiltered.shape == curve_filtered.shape and curve_unfiltered.ndim == 2 and len(curve_unfiltered) > 100
    assert np.all(np.isfinite(line.lags_raw)) and np.all(np.abs(line.corrs) >= REJECT)      # nothing rejected: lags_raw (which shares its memory with lags until the median) is the raw data
    inside = np.flatnonzero((curve_unfiltered[:, 0] >= line.times[0]) & (curve_unfiltered[:, 0] <= line.times[-1]))
    n_curve = len(curve_unfiltered)
    rows = np.unique(np.concatenate((np.arange(max(0, inside[0] - 20), min(n_curve, inside[-1] + 21)), np.arange(0, n_curve, 97),
                                     np.arange(n_curve - 5, n_curve))))
    near = np.flatnonzero((lag_curve0[:, 0] >= line.times[0]) & (lag_curve0[:, 0] <= line.times[-1]))
    lag_curve0 = lag_curve0[near[0] - 3:near[-1] + 4]
    assert lag_curve0[0, 0] < line.times[0] and lag_curve0[-1, 0] > line.times[-1]
    assert np.array_equal(sample_lags, np.interp(line.times, lag_curve0[:, 0], lag_curve0[:, 1]))
    curve_unfiltered, curve_filtered = curve_unfiltered[rows], curve_filtered[rows]
    save("azimuth", curve_len=np.array(n_curve), curve_rows=rows, sr=np.array(sr), hop=np.array(hop), smoothing=np.array(cfg["smoothing"]), duration=np.array(c.duration),
         len_ref=np.array(len(ref_sig)), len_src=np.array(len(src_sig)), t0=np.array(t0), t1=np.array(t1),
         lower=np.array(float(lower)), upper=np.array(float(upper)), dur=np.array(DUR), overlap=np.array(OVERLAP),
         reject=np.array(REJECT), bands=np.array(BANDS, dtype=np.float64), lag_curve0=lag_curve0,
         sample_times=np.array(line.times, dtype=np.float64), sample_lags=sample_lags,
         lags_raw=np.array(line.lags_raw, dtype=np.float64), lags=np.array(line.lags, dtype=np.float64),
         corrs=np.array(line.corrs, dtype=np.float64), ref_geom=np.array(geoms[0], dtype=np.int64),
         src_geom=np.array(geoms[1], dtype=np.int64), curve_unfiltered=curve_unfiltered, curve_filtered=curve_filtered)
    print(f"{W} windows, lags {line.lags.min():.6f} .. {line.lags.max():.6f} s, |corr| {np.abs(line.corrs).min():.3f} .. "
          f"{np.abs(line.corrs).max():.3f}; curve {curve_unfiltered.shape} {curve_unfiltered.dtype}")


if __name__ == "__main__":
    main()
