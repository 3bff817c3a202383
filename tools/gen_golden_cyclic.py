"""Fixture of the cyclic wow analysis, computed by the REFERENCE's own script (build container only).

    python tools/gen_golden_cyclic.py --ref /path/to/pyaudiorestoration

experiments/cyclic_wow.py is a script: its top level reads ../samples/cyclic_pilot+n.wav, which the reference does not ship.  This
tool synthesises a pilot, writes it into a temporary tree where that relative path resolves, and executes the script itself there,
unchanged, through oracle/ref_gui.py's import hook (matplotlib and the other absent packages are stand-ins; io_ops.read_file is
swapped for this project's WAV reader, as soundfile is absent).  The script's globals are kept; nothing of the script is copied.

The pilot (tests/golden/cyclic_pilot.wav, mono, 16 bit, 22050 Hz, 12 s): a 700 Hz tone with a cyclic speed error of +-0.5 % at the
rotation period 60 / 45.6 s and a second harmonic of the cycle at half that depth, plus low noise.  At the script's hop of 128 samples the
rotation is about 226.7 frames where the script's initial guess for 45 rpm is 229: the search has to move off its starting point.

Only data is stored, in tests/golden/cyclic.npz:

  sr, fft_size, hop, rpm, tolerance, pilot_hz, tolerance_st, frames_per_rotation_init, d      the parameters
  times, freqs, frame_0, frame_1      PeakTracker's track
  results (2 d, 2), best (frames_per_rotation, delta), avg      the search and the winning fold
  cycle_duration, rpm_measured, printed      the figures the script prints and the lines themselves

Deterministic: running it twice writes identical files."""
import argparse
import contextlib
import io
import os
import runpy
import shutil
import sys
import tempfile
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gen_golden_expander import GOLDEN, save  # noqa: E402
from oracle import ref_gui  # noqa: E402

SR, SECONDS, PILOT_HZ, TRUE_RPM = 22050, 12.0, 700.0, 45.6


def pilot():
    """int16 samples of the pilot tone"""
    t = np.arange(int(SR * SECONDS)) / SR
    period = 60.0 / TRUE_RPM
    speed = 1.0 + 0.005 * np.sin(2 * np.pi * t / period) + 0.0025 * np.sin(4 * np.pi * t / period + 2.0)
    phase = 2 * np.pi * PILOT_HZ * np.cumsum(speed) / SR
    x = 0.5 * np.sin(phase) + 0.0005 * np.random.default_rng(45).standard_normal(len(t))
    return np.rint(x * 32767.0).astype("<i2")


def write_wav16(path, samples):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(SR)
        w.writeframes(samples.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (pyaudiorestoration)")
    a = ap.parse_args()
    ref_gui.import_reference_gui(a.ref)
    from util import fourier, io_ops
    from pyaudiorestoration_amd import io_ops as our_io

    def pyfftw_absent(*args):                         # its stand-in module cannot compute: the backend fails as without the library
        raise ImportError("pyfftw is not installed")
    fourier.pyfftw_rfft2 = pyfftw_absent
    io_ops.read_file = our_io.read_file

    golden_wav = os.path.join(GOLDEN, "cyclic_pilot.wav")
    write_wav16(golden_wav, pilot())
    tmp = tempfile.mkdtemp()
    cwd = os.getcwd()
    out = io.StringIO()
    try:
        os.makedirs(os.path.join(tmp, "samples"))
        os.makedirs(os.path.join(tmp, "experiments"))
        shutil.copyfile(golden_wav, os.path.join(tmp, "samples", "cyclic_pilot+n.wav"))
        os.chdir(os.path.join(tmp, "experiments"))
        with contextlib.redirect_stdout(out), np.errstate(all="ignore"):
            g = runpy.run_path(os.path.join(a.ref, "experiments", "cyclic_wow.py"), run_name="__main__")
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp)
    track = g["track"]
    printed = [ln for ln in out.getvalue().splitlines() if not ln.startswith("Testing cycle length")]
    print("\n".join(printed))
    print(f"spectrum {g['spectrum'].shape} {g['spectrum'].dtype}, track {len(track.freqs)} frames [{track.frame_0}, {track.frame_1}), "
          f"init {g['frames_per_rotation_init']}, d {g['d']}")
    save("cyclic",
         sr=np.array(g["sr"]), fft_size=np.array(g["fft_size"]), hop=np.array(g["fft_hop"]), rpm=np.array(g["rpm"]),
         tolerance=np.array(g["tolerance"]), pilot_hz=np.array(PILOT_HZ), tolerance_st=np.array(10),
         frames_per_rotation_init=np.array(g["frames_per_rotation_init"]), d=np.array(g["d"]),
         times=np.asarray(track.times), freqs=np.asarray(track.freqs), frame_0=np.array(track.frame_0), frame_1=np.array(track.frame_1),
         results=np.asarray(g["results"]), best=np.array([g["frames_per_rotation"], g["delta"]]), avg=np.asarray(g["avg"]),
         cycle_duration=np.array(g["cycle_duration"]), rpm_measured=np.array(60.0 / g["cycle_duration"]), printed=np.array(printed))


if __name__ == "__main__":
    main()
