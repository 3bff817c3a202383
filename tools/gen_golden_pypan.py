"""Fixture of the stereo balance tool, computed by the REFERENCE's own code (build container only).

    python tools/gen_golden_pypan.py --ref /path/to/pyaudiorestoration

The reference's modules are imported through oracle/ref_gui.py's import hook (stand-ins for the absent PyQt5 / vispy packages).
No file under tests/golden has two different channels (every one is mono), so the input is tests/pan_np.stereo_tape(seed): a
common programme with a different slowly varying gain per channel plus independent noise, from the generators of
tests/inputs.py.  On a stand-in canvas whose two spectra carry what the reference's FourierThread stores
(fourier.get_mag(channel, fft_size, hop, "blackmanharris", zeropad), through whichever backend of its chain works), it runs unchanged

  pypan_gui.Canvas.on_mouse_release, `Shift` branch (:78-104), once per box
  markers.PanLine.update (util/markers.py:711-727) over the markers it pushed (those with a finite factor)
  pypan_gui.Canvas.run_resample (:53-58), io_ops.read_file / write_file swapped for in-memory ones

The integers of a box are locals of the method: the spectra are handed over as an ndarray subclass that records the slices the
method takes of them, and np.interp is wrapped for the length of run_resample to keep `af`; nothing of the reference is restated.
Only data is stored, in tests/golden/pypan.npz:

  seed, sr, n, fft_size, fft_overlap, hop, duration, spectra_dtype, backend
  boxes (a_t, a_f, b_t, b_f), cells (bL, bU, first, last), fac            zeropad 1, every box
  boxes_zp2, cells_zp2, fac_zp2, zeropad2                                 the same for two boxes at zero-padding 2
  small_box, small_L, small_R                                             index of one small box, the reference's own cells [bins][frames]
  markers                                                                 PanSample.to_cfg() rows in the order pushed
  pan_data                                                                PanLine.data, whole (a few hundred rows; nothing to thin)
  af_idx, af                                                              rows of run_resample's np.interp around every knot, the ends
  out_idx, out, out_dtype                                                 samples of the array handed to write_file, and its dtype
  s0                                                                      |fac - fsum(small cells) / cnt| / fac (tests/pan_np.py B_ref)

Deterministic: running it twice writes identical files."""
import argparse
import math
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pan_np  # noqa: E402
from gen_golden_expander import save  # noqa: E402
from oracle import ref_gui  # noqa: E402

BOXES = (((0.4, 300.0), (1.0, 4000.0)),          # the usual case
         ((0.0, 50.0), (0.5, 12000.0)),          # a start time of exactly 0; the upper frequency beyond sr // 2 - 1
         ((2.5, 2000.0), (9.0, 500.0)),          # an end time beyond the file; frequencies clicked high to low
         ((1.5, 1000.0), (1.56, 1400.0)),        # the small box whose cells are stored
         ((2.2, 5000.0), (1.8, 800.0)),          # clicked right to left
         ((1.0, 3000.0), (1.001, 3000.0)),       # collapses to an empty slice: nanmean gives NaN
         ((0.7, 0.2), (0.9, 30.0)))              # frequencies under 1 Hz: clamps to bin 1
SMALL = 3
BOXES_ZP2 = (BOXES[0], BOXES[3])
ZEROPAD2 = 2


class Recording(np.ndarray):
    """an array that remembers the keys it was indexed with"""
    def __getitem__(self, key):
        if isinstance(key, tuple) and all(isinstance(k, slice) for k in key):
            self.taken.append(tuple((k.start, k.stop) for k in key))
        return np.asarray(super().__getitem__(key))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (pyaudiorestoration)")
    a = ap.parse_args()
    _, _, markers, _ = ref_gui.import_reference_gui(a.ref)
    import pypan_gui as P
    from util import fourier

    used = []

    def pyfftw_absent(*args):                         # its stand-in module cannot compute: the backend fails as without the library
        raise ImportError("pyfftw is not installed")
    fourier.pyfftw_rfft2 = pyfftw_absent
    for name in ("torch_rfft2", "pyfftw_rfft2", "np_rfft_pick"):
        def rec(*args, _fn=getattr(fourier, name), _name=name):
            r = _fn(*args)
            used.append(_name)
            return r
        setattr(fourier, name, rec)

    sig = pan_np.stereo_tape()
    sr, n = pan_np.SR, len(sig)
    fft_size, overlap = pan_np.FFT_SIZE, pan_np.FFT_OVERLAP
    hop = fft_size // overlap

    def canvas(zeropad):
        c = ref_gui.fake_canvas(sr, fft_size, hop, duration=n / sr)
        c.filenames = ["tape.wav"]
        c.spec_view = ref_gui._Anything()                 # PanSample's rectangle wants a scene to hang in: any object
        c.spectra = []
        for ch in (0, 1):
            mag = fourier.get_mag(sig[:, ch], fft_size, hop, "blackmanharris", zeropad)       # qt_threads.FourierThread.run
            arr = np.asarray(mag).view(Recording)
            arr.taken = []
            c.spectra.append(ref_gui.NS(key="k", fft_storage={"k": arr}, mel_transform=ref_gui._Anything()))
        c.px_to_spectrum = lambda click: click
        c.pushed = []
        c.props.undo_stack = ref_gui.NS(push=lambda action: c.pushed.extend(action.traces))
        return c

    def measure(c, boxes):
        cells, facs = [], []
        for a_, b_ in boxes:
            for s in c.spectra:
                s.fft_storage["k"].taken.clear()
            event = ref_gui.NS(trail=lambda a_=a_: [a_], pos=b_, button=1, modifiers=("Shift",))
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                P.Canvas.on_mouse_release(c, event)
            tl, tr = (s.fft_storage["k"].taken for s in c.spectra)
            assert len(tl) == 1 and tl == tr, (tl, tr)
            (bl, bu), (f0, f1) = tl[0]
            cells.append((bl, bu, f0, f1))
            facs.append(float(c.pushed[-1].pan))
        return np.array(cells, dtype=np.int64), np.array(facs, dtype=np.float64)

    c = canvas(1)
    cells, fac = measure(c, BOXES)
    L, R = (np.asarray(s.fft_storage["k"]) for s in c.spectra)
    bl, bu, f0, f1 = cells[SMALL]
    small_L, small_R = np.array(L[bl:bu, f0:f1]), np.array(R[bl:bu, f0:f1])
    exact, cnt0, _ = pan_np.fsum_mean(small_L / small_R)
    s0 = abs(fac[SMALL] - exact) / abs(fac[SMALL])

    # the line and the resampled file, from the finite markers in the order they were pushed
    keep = [m for m in c.pushed if math.isfinite(m.pan)]
    for m in keep:
        m.initialize()                                   # AddAction.redo: the marker joins the canvas' markers
    assert len(c.markers) == len(keep) >= 4
    c.pan_line = markers.PanLine(c)
    c.pan_line.update()
    pan_data = np.array(c.pan_line.data)
    written, interps = {}, []
    old_r, old_w, old_i = P.io_ops.read_file, P.io_ops.write_file, np.interp

    def interp(*args, **kw):
        r = old_i(*args, **kw)
        interps.append(r)
        return r
    P.io_ops.read_file = lambda path: (sig, sr, 2)
    P.io_ops.write_file = lambda path, data, sr_, ch, suffix="_out": written.update(data=np.array(data), ch=ch, suffix=suffix)
    np.interp = interp
    try:
        P.Canvas.run_resample(c)
    finally:
        P.io_ops.read_file, P.io_ops.write_file, np.interp = old_r, old_w, old_i
    assert len(interps) == 1 and written["ch"] == 1 and written["suffix"] == "_out" and written["data"].shape == (n,)
    af = interps[0]
    knots = [int(round(m.t * sr)) for m in keep]
    idx = np.unique(np.clip(np.concatenate([np.arange(k - 8, k + 9) for k in knots] + [np.arange(16), np.arange(n - 16, n),
                                                                                       np.arange(0, n, 13)]), 0, n - 1))
    c2 = canvas(ZEROPAD2)
    cells2, fac2 = measure(c2, BOXES_ZP2)

    save("pypan", seed=np.array(pan_np.SEED), sr=np.array(sr), n=np.array(n), fft_size=np.array(fft_size), fft_overlap=np.array(overlap),
         hop=np.array(hop), duration=np.array(c.duration), spectra_dtype=np.array(str(L.dtype)), backend=np.array(sorted(set(used))),
         boxes=np.array([(a_[0], a_[1], b_[0], b_[1]) for a_, b_ in BOXES], dtype=np.float64), cells=cells, fac=fac,
         boxes_zp2=np.array([(a_[0], a_[1], b_[0], b_[1]) for a_, b_ in BOXES_ZP2], dtype=np.float64), cells_zp2=cells2, fac_zp2=fac2,
         zeropad2=np.array(ZEROPAD2), small_box=np.array(SMALL), small_L=small_L, small_R=small_R,
         markers=np.array([m.to_cfg() for m in keep], dtype=np.float64), pan_data=pan_data, af_idx=idx.astype(np.int32), af=af[idx],
         out_idx=idx.astype(np.int32), out=written["data"][idx], out_dtype=np.array(str(written["data"].dtype)), s0=np.array(s0))
    print(f"backend {sorted(set(used))}, spectra {L.dtype} {L.shape}; cells {cells.tolist()}; fac {fac.tolist()}; zp2 {cells2.tolist()} "
          f"{fac2.tolist()}; small box {cnt0} cells, s0 = {s0:.3e}; line {pan_data.shape} {pan_data.dtype}; out {written['data'].dtype}")


if __name__ == "__main__":
    main()
