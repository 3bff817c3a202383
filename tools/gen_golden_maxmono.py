"""Fixtures of MaxMono (dropouts_gui.MainWindow.process_max_mono), computed by the REFERENCE's own code (build container only).

    python tools/gen_golden_maxmono.py [--ref /path/to/pyaudiorestoration]

MainWindow.process_max_mono is called as a plain function on a stand-in window that carries only the file list it reads.  The
reference's io_ops.read_file / write_file are swapped for in-memory ones; its modules are imported through oracle/ref_gui.py's
import hook.  Only arrays the reference computed are stored: tests/golden/maxmono.npz (under 1 MB; the outputs as strided
samples).  Deterministic: running it twice writes identical files.

The input is nr_signal.wav with its copy rolled by 1789 samples as the second channel (the renoiser fixture's stereo stand-in).
Per setting (fft/hop): both masks (|D_L| > |D_R| and |D_L| < |D_R|) as packed bits of the (frames, bins) STFTs, from the same
transform of the same padded channels process_max_mono takes; both written outputs cast to float32 as the FLOAT file holds
them; the output peaks; the transform backend the reference used and the dtype of its spectra.  Without pyfftw or torch the
reference's transform comes out complex128: the golden decisions are float64 decisions (spec_dtype says so)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = os.path.join(ROOT, "tests", "golden")

from gen_golden_expander import save  # noqa: E402
from oracle import ref_gui  # noqa: E402
from pyaudiorestoration_amd import io_ops as our_io  # noqa: E402   (WAV decoding of the sample file only)

SETTINGS = ((2048, 512), (512, 64), (64, 16))
STEREO_SHIFT = 1789            # samples: the second channel is nr_signal delayed (circularly) by this much
STRIDE = 4                     # every STRIDE-th output sample is stored


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    ref_gui.import_reference_gui(a.ref)
    import dropouts_gui as G
    from util import fourier

    used = []
    def pyfftw_absent(*args):
        raise ImportError("pyfftw is not installed")
    fourier.pyfftw_rfft2 = pyfftw_absent
    for name in ("torch_rfft2", "pyfftw_rfft2", "np_rfft_pick"):
        fn = getattr(fourier, name)
        def rec(*args, _fn=fn, _name=name):
            r = _fn(*args)
            used.append(_name)
            return r
        setattr(fourier, name, rec)

    sig, sr, _ = our_io.read_file(os.path.join(GOLDEN, "nr_signal.wav"))
    sig = sig if sig.ndim == 2 else sig[:, None]
    stereo = np.concatenate([sig, np.roll(sig, STEREO_SHIFT, axis=0)], axis=1).astype(np.float32)
    n = len(stereo)
    written = {}
    G.io_ops.read_file = lambda path: (np.array(stereo, dtype=np.float32), sr, 2)
    G.io_ops.write_file = lambda path, data, rate, ch, suffix="_out": written.__setitem__(suffix, (np.array(data), path, rate, ch))

    out = {"sr": np.array(sr), "signal_sum": np.array(float(np.sum(sig, dtype=np.float64))), "stereo_shift": np.array(STEREO_SHIFT),
           "stride": np.array(STRIDE), "settings": np.array(SETTINGS, dtype=np.int64)}
    dtypes = set()
    for fft, hop in SETTINGS:
        k = f"{fft}_{hop}"
        win = ref_gui.NS(file_names=["tape.wav"], names_to_full_paths={"tape.wav": "tape.wav"})
        written.clear()
        with np.errstate(all="ignore"):
            G.MainWindow.process_max_mono(win, fft, hop)
            # the masks process_max_mono selected by, from the same STFTs of the same padded channels
            pad = fourier.fix_length(stereo, n + fft // 2, axis=0)
            D_L = np.array(fourier.stft(pad[:, 0], n_fft=fft, step=hop))
            D_R = np.array(fourier.stft(pad[:, 1], n_fft=fft, step=hop))
        dtypes.add(str(D_L.dtype))
        assert sorted(written) == ["max", "min"], sorted(written)
        for op, mask in (("max", np.abs(D_L) > np.abs(D_R)), ("min", np.abs(D_L) < np.abs(D_R))):
            y, path, rate, ch = written[op]
            assert (path, rate, ch) == ("tape.wav", sr, 1) and y.shape == (n,), (path, rate, ch, y.shape)
            # the reference redoes exactly this selection: its output is the ISTFT of np.where(mask, D_L, D_R)
            again = np.asarray(fourier.istft(np.where(mask, D_L, D_R), length=n, hop_length=hop))
            assert np.array_equal(again, y), (fft, hop, op)
            y32 = y.astype(np.float32)                                 # subtype FLOAT
            out[f"{k}_mask_{op}"] = np.packbits(mask.T.reshape(-1))     # (frames, bins) order
            out[f"{k}_y_{op}"] = y32[::STRIDE].copy()
            out[f"{k}_peak_{op}"] = np.array(float(np.max(np.abs(y32))))
        out[f"{k}_frames"] = np.array(D_L.shape[1])
        tie = int(np.sum(np.abs(D_L) == np.abs(D_R)))
        print(f"{fft}/{hop}: {D_L.shape[1]} frames x {D_L.shape[0]} bins, L louder in {np.mean(np.abs(D_L) > np.abs(D_R)):.3f}, "
              f"{tie} ties, peaks {out[f'{k}_peak_max'][()]:.4f} / {out[f'{k}_peak_min'][()]:.4f}")
    assert len(dtypes) == 1, dtypes
    out["backend"] = np.array(sorted(set(used)))
    out["spec_dtype"] = np.array(dtypes.pop())
    print("backend", out["backend"], "spectra", out["spec_dtype"])
    save("maxmono", **out)


if __name__ == "__main__":
    main()
