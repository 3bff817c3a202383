"""Fixture of the zero-crossing flutter analysis, computed by the REFERENCE's own script (build container only).

    python tools/gen_golden_zerocrossing.py --ref /path/to/pyaudiorestoration

experiments/zerocrossing_wow.py is a script: its top level reads ../samples/flutter_192.flac and ../samples/flutter.flac, which
the reference does not ship, and draws two curves per file with matplotlib.  This tool synthesises two short pilots, writes them
as FLAC (tests/flac_writer.py) into a temporary tree under those names, and executes the script itself, unchanged, through
oracle/ref_gui.py's import hook: io_ops.read_file is swapped for this project's reader and resolves the two file names in the
temporary tree (soundfile is absent), the stand-in pyplot's `plot` records its arguments, the script's print goes to a buffer.
Nothing of the script is copied; only arrays it computed are stored.

The pilots (16 bit mono): `a` 4 kHz at 192 kHz, 0.2 s, flutter +-2 % at 23 Hz; `b` 3 kHz at 44.1 kHz, 0.25 s, +-3 % at 17 Hz; both
with a little noise (tests/zerocross_np.pilot).

tests/golden/zerocrossing.npz, per pilot k in (a, b):

  k_signal (int16), k_sr, k_crossings (recomputed as the script does: the sign changes of the float32 samples)
  k_raw_t, k_raw_f      the arguments of the script's first plot call: crossings[:n] / sr, sr / 2 / deltas (float32)
  k_t, k_f              those of its second: the smoothed curve (float64)
  k_size                the script's `size` (len(win_sq), the second number it prints)
  k_mean                np.mean(deltas), the fourth number it prints, as printed
  k_quotient            sr / 100 / ((last - first) / n) in float64: its distance to an integer is asserted >= 1e-3 here, so
                        zerocrossing_wow.smoothing_span and the reference's float32 mean agree on these fixtures

Deterministic: running it twice writes identical files."""
import argparse
import contextlib
import io
import os
import runpy
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import flac_writer  # noqa: E402
import zerocross_np as Z  # noqa: E402
from gen_golden_expander import save  # noqa: E402
from oracle import ref_gui  # noqa: E402

# key -> (the script's file name, sr, pilot Hz, seconds, flutter depth, flutter Hz, noise, seed)
PILOTS = {"a": ("flutter_192.flac", 192000, 4000.0, 0.2, 0.02, 23.0, 0.001, 7),
          "b": ("flutter.flac", 44100, 3000.0, 0.25, 0.03, 17.0, 0.001, 8)}


def pilot16(key):
    _, sr, hz, seconds, depth, f_hz, noise, seed = PILOTS[key]
    assert seconds <= 0.25
    return np.rint(Z.pilot(sr, hz, seconds, depth, f_hz, noise, seed).astype(np.float64) * 32767.0).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (pyaudiorestoration)")
    a = ap.parse_args()
    ref_gui.import_reference_gui(a.ref)
    import matplotlib
    from util import io_ops
    from pyaudiorestoration_amd import io_ops as our_io

    plots = []
    matplotlib.pyplot.plot = lambda *args, **kw: plots.append((tuple(np.array(v) for v in args), kw))
    tmp = tempfile.mkdtemp()
    io_ops.read_file = lambda path: our_io.read_file(os.path.join(tmp, "samples", os.path.basename(path)))
    out = io.StringIO()
    try:
        os.makedirs(os.path.join(tmp, "samples"))
        for key, spec in PILOTS.items():
            with open(os.path.join(tmp, "samples", spec[0]), "wb") as f:
                f.write(flac_writer.encode_flac(pilot16(key).astype(np.int64), spec[1], 16, blocksize=4096, kind="fixed", order=2))
        with contextlib.redirect_stdout(out), np.errstate(all="ignore"):
            runpy.run_path(os.path.join(a.ref, "experiments", "zerocrossing_wow.py"), run_name="__main__")
    finally:
        shutil.rmtree(tmp)
    printed = [ln.split() for ln in out.getvalue().splitlines() if len(ln.split()) == 4]
    assert len(plots) == 4 and len(printed) == 2, (len(plots), out.getvalue())
    arrays = {}
    for k, key in enumerate(PILOTS):
        sr = PILOTS[key][1]
        sig = pilot16(key)
        x = (sig / 32768.0).astype(np.float32)                   # the reader's scaling
        positive = x > 0
        crossings = np.where(positive[1:] != positive[:-1])[0]
        (raw_t, raw_f), raw_kw = plots[2 * k]
        (t, f), kw = plots[2 * k + 1]
        assert raw_kw.get("label") == "raw" and kw.get("label") == "deltas_conv"
        n = len(crossings) - 1
        assert len(raw_t) == len(t) == n and np.array_equal(raw_t, crossings[:n] / sr), "the script saw other crossings"
        n_printed, size, _, mean = printed[k]
        assert int(n_printed) == n
        quotient = sr / 100 / ((int(crossings[-1]) - int(crossings[0])) / n)
        assert abs(quotient - round(quotient)) >= 1e-3 and int(quotient) == int(size), (quotient, size)
        print(f"{key}: {len(sig)} samples at {sr} Hz, {n + 1} crossings, size {size}, quotient {quotient!r}, mean period {mean}")
        arrays.update({f"{key}_signal": sig, f"{key}_sr": np.array(sr), f"{key}_crossings": crossings.astype(np.int64),
                       f"{key}_raw_t": raw_t, f"{key}_raw_f": raw_f, f"{key}_t": t, f"{key}_f": f, f"{key}_size": np.array(int(size)),
                       f"{key}_mean": np.array(mean), f"{key}_quotient": np.array(quotient)})
    save("zerocrossing", **arrays)


if __name__ == "__main__":
    main()
