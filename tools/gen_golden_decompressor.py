"""Fixture of the dynamics matcher, computed by the REFERENCE's own code (build container only).

    python tools/gen_golden_decompressor.py [--ref /path/to/pyaudiorestoration]

experiments/decompressor_cmd.process is run unchanged on two in-memory files: the reference's modules are imported through
oracle/ref_gui.py's import hook (stand-ins for the absent soundfile / matplotlib packages), the module's `sf` is replaced by the
stand-ins below (SoundFile hands out the arrays, write records what it is given) and os.path.isfile says yes to the two names.
Only the input and arrays the reference computed are stored: tests/golden/decompressor.npz

  x_i16, roll, gain_values, gain_run, sr   the input (tests/dynamics_np.golden_input rebuilds src and ref from them, exactly)
  out                                      the float64 array the reference hands to sf.write, at the rows dynamics_np.golden_rows
  out_peak                                 max |out| over the whole file
Deterministic: running it twice writes identical files."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dynamics_np as D  # noqa: E402
from gen_golden_expander import save  # noqa: E402
from oracle import ref_gui  # noqa: E402


class FakeSoundFiles:
    """what decompressor_cmd.py reads of the soundfile module: SoundFile(name) with .read(always_2d, dtype), .samplerate,
    .channels, and write(name, data, sr, subtype)"""

    def __init__(self, files, sr):
        self.files, self.sr, self.written = files, sr, {}
        outer = self

        class SoundFile:
            def __init__(self, name):
                self.data = outer.files[name]
                self.samplerate, self.channels = outer.sr, self.data.shape[1]

            def read(self, always_2d=True, dtype="float32"):
                assert always_2d and dtype == "float32"
                return np.array(self.data, dtype=np.float32)
        self.SoundFile = SoundFile

    def write(self, name, data, sr, subtype=None):
        self.written.update(name=name, data=np.array(data), sr=sr, subtype=subtype)


def run_reference(mod, src, ref, sr):
    """decompressor_cmd.process on two in-memory files -> the FakeSoundFiles that recorded the write"""
    fake = FakeSoundFiles({"src.wav": src, "ref.wav": ref}, sr)
    old_sf, old_isfile = mod.sf, os.path.isfile
    mod.sf, os.path.isfile = fake, lambda p: p in fake.files or old_isfile(p)
    try:
        with np.errstate(all="ignore"):
            mod.process("src.wav", "ref.wav")
    finally:
        mod.sf, os.path.isfile = old_sf, old_isfile
    return fake


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    ref_gui.import_reference_gui(a.ref)
    from experiments import decompressor_cmd as mod

    g = dict(x_i16=D.make_golden_source(), roll=np.array(D.GOLDEN_ROLL), gain_values=D.GOLDEN_GAIN_VALUES, gain_run=np.array(D.GOLDEN_GAIN_RUN),
             sr=np.array(D.SR))
    src, ref = D.golden_input(g)
    assert np.array_equal(ref.astype(np.float64), src.astype(np.float64) * np.repeat(D.GOLDEN_GAIN_VALUES, D.GOLDEN_GAIN_RUN)[:len(src), None])
    fake = run_reference(mod, src, ref, D.SR)
    w = fake.written
    assert w["name"] == "src.wavdecompressed.wav" and w["subtype"] == "FLOAT" and w["sr"] == D.SR and w["data"].dtype == np.float64
    out = w["data"]
    # the restatement the tests use equals the reference bit for bit over the whole file
    mine = D.match_dynamics_np(src, ref, D.SR)
    assert np.array_equal(mine.view(np.uint64), out.view(np.uint64)), "tests/dynamics_np.py no longer restates the reference"
    n = len(src)
    rows = D.golden_rows(n)
    g["out"] = out[rows]
    g["out_peak"] = np.array(np.max(np.abs(out)))
    print(f"n {n}, frames {D.n_frames(n, D.HOP)}, rows stored {len(rows)}, peak {float(g['out_peak']):.6g}")
    save("decompressor", **g)
    assert os.path.getsize(D.GOLDEN) < 1_000_000


if __name__ == "__main__":
    main()
