"""Fixtures of the hum speed analysis (humspeed_gui.MainWindow), computed by the REFERENCE's own code (build container only).

    python tools/gen_golden_humspeed.py [--ref /path/to/pyaudiorestoration]

MainWindow.track_to and MainWindow.on_hum_param_changed are called unbound, as plain functions, on a stand-in window that
carries only the attributes they read (spin boxes reduced to attribute bags with a value(), the label to a recorder, the
clipboard and the plot to oracle/ref_gui.py's throw-away stand-ins).  The reference's modules are imported through
oracle/ref_gui.py's import hook.  Only arrays the reference computed, and the small synthetic spectra they were computed from,
are stored: tests/golden/humspeed.npz (about 20 KB).  Deterministic: running it twice writes identical files.

Spectra are 2049 bins (a 4096-point transform).  Cases:
  inside      a hum peak 1.4 % off, well inside the tolerance
  rejected    the highest bin of the band is its first one, on the slope of a louder peak outside: the parabola lands
              outside the tolerance ("hum was not close enough")
  first_bin   a peak on the band's first bin that the parabola moves back inside the tolerance
  coarse      8 kHz sample rate: 1.95 Hz bins, the band is four bins wide
  harmonics3  on_hum_param_changed with three harmonics, all found
  harmonics2  on_hum_param_changed with the default two harmonics, the first harmonic missing (rejected): order of the rest"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gen_golden_expander import save  # noqa: E402
from oracle import ref_gui  # noqa: E402

FFT = 4096
BINS = FFT // 2 + 1


def floor_spectrum(seed):
    """-90 dB, with a seeded +-3 dB ripple over the 256 bins the searches look at (the flat rest compresses to nothing)"""
    spec = np.full(BINS, -90.0)
    spec[:256] += 3.0 * np.random.default_rng(seed).standard_normal(256)
    return spec


def add_peak(spec, pos, height=-30.0, width=0.9):
    """a smooth bump centred on the (fractional) bin pos"""
    b = np.arange(BINS)
    return np.maximum(spec, height - ((b - pos) / width) ** 2 * 6.0)


def cases():
    c = {}
    c["inside"] = dict(spectrum=add_peak(floor_spectrum(1), 50.7), sr=4096, tol=8, xpos=50.0, base=50, harm=2)
    s = floor_spectrum(2)
    s[46], s[45], s[44], s[47] = -40.0, -35.0, -30.0, -48.0          # the slope of a peak below the band
    c["rejected"] = dict(spectrum=s, sr=4096, tol=8, xpos=50.0, base=50, harm=2)
    s = floor_spectrum(3)
    s[45], s[46], s[47], s[48] = -70.0, -30.0, -30.5, -60.0          # vertex near 46.49: 50 / 46.49 is 7.6 % off
    c["first_bin"] = dict(spectrum=s, sr=4096, tol=8, xpos=50.0, base=50, harm=2)
    c["coarse"] = dict(spectrum=add_peak(floor_spectrum(4), 60.4 * FFT / 8000), sr=8000, tol=8, xpos=60.0, base=60, harm=2)
    s = floor_spectrum(5)
    for k in range(1, 5):
        s = add_peak(s, 50.7 * k, -30.0 - 4 * k)
    c["harmonics3"] = dict(spectrum=s, sr=4096, tol=8, xpos=None, base=50, harm=3)
    s = floor_spectrum(6)
    s = add_peak(add_peak(s, 49.2), 147.6, -41.0)
    s[92], s[91], s[90], s[93] = -40.0, -35.0, -30.0, -48.0          # 100 Hz: rejected like the case above
    c["harmonics2"] = dict(spectrum=s, sr=4096, tol=8, xpos=None, base=50, harm=2)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    ref_gui.import_reference_gui(a.ref)
    import humspeed_gui as H
    from util import fourier
    NS = ref_gui.NS

    out = {"cases": np.array(sorted(cases())), "fft_size": np.array(FFT)}
    for name, c in cases().items():
        texts = []
        w = NS(freqs=fourier.fft_freqs(FFT, c["sr"]), spectrum=c["spectrum"], sr=c["sr"], fft_size=FFT, marker_freqs=[], marker_dBs=[],
               ratios=[], hum_freqs=np.arange(c["base"], c["base"] + c["base"] * c["harm"] + 1, c["base"]),
               s_tolerance=NS(value=lambda c=c: c["tol"]), s_base_hum=NS(value=lambda c=c: c["base"]),
               s_num_harmonies=NS(value=lambda c=c: c["harm"]), l_result=NS(setText=texts.append), cb=ref_gui._Anything(),
               plot=lambda: None)
        ref_gui._bind(w, H.MainWindow, "track_to", "on_hum_param_changed")
        if c["xpos"] is None:
            w.on_hum_param_changed()
        else:
            w.track_to(c["xpos"])
        out[f"{name}_spectrum"] = np.asarray(c["spectrum"], dtype=np.float64)
        out[f"{name}_params"] = np.array([c["sr"], c["tol"], -1.0 if c["xpos"] is None else c["xpos"], c["base"], c["harm"]], dtype=np.float64)
        out[f"{name}_hum_freqs"] = np.asarray(w.hum_freqs)
        out[f"{name}_marker_freqs"] = np.array(w.marker_freqs, dtype=np.float64)
        out[f"{name}_marker_dBs"] = np.array(w.marker_dBs, dtype=np.float64)
        out[f"{name}_ratios"] = np.array(w.ratios, dtype=np.float64)
        out[f"{name}_texts"] = np.array(texts if texts else [""])
        print(f"{name}: freqs {w.marker_freqs} ratios {w.ratios} label {texts}")
    save("humspeed", **out)


if __name__ == "__main__":
    main()
