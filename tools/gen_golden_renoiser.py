"""Fixtures of the renoiser (renoiser_gui.Canvas), computed by the REFERENCE's own code (build container only).

    python tools/gen_golden_renoiser.py [--ref /path/to/pyaudiorestoration]

Canvas.redraw_plot / get_mask_fac / run_resample / load_noise_profile / on_mouse_release are called as plain functions on a
stand-in canvas that carries only the attributes they read (the GUI's widgets reduced to attribute bags, the plot objects to
oracle/ref_gui.py's throw-away stand-ins).  The reference's io_ops.read_file / write_file are swapped for in-memory ones, the
file dialog returns the noise file's name, and resampy.resample -- not installed -- is the identity, which is what it computes
at equal rates (every noise file here is at the signal's rate; the generator asserts it).  The reference's modules are imported
through oracle/ref_gui.py's import hook.  Only arrays the reference computed are stored: tests/golden/renoiser.npz (under 1 MB;
long outputs as strided samples).  Deterministic: running it twice writes identical files.

Per setting: the noise profile, the final profile, the mask (1 = bin passes) as packed bits of the (frames, bins) STFT of
run_resample, the bins within 1e-3 dB of their threshold (frame, bin and dB) and the written output."""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = os.path.join(ROOT, "tests", "golden")

from gen_golden_expander import save  # noqa: E402
from oracle import ref_gui  # noqa: E402
from pyaudiorestoration_amd import io_ops as our_io  # noqa: E402   (WAV decoding of the sample files only)

NEAR_DB = 1e-3
# name: (fft, hop, gain, overhead, curve, profile source, stereo, output stride)
SETTINGS = {
    "default": (2048, 512, 12.0, 3.0, None, "noise", False, 1),
    "hop128": (2048, 128, 12.0, 3.0, None, "noise", False, 2),
    "gate": (1024, 256, -20.0, 26.0, [[1, 0.0], [3000, -6.0], [22050, 4.0]], "noise", False, 4),
    "big": (16384, 4096, 12.0, 3.0, None, "noise", False, 4),
    "noprofile": (2048, 512, 12.0, 3.0, None, "none", False, 4),
    "select": (2048, 512, 12.0, 3.0, None, "select", False, 4),
    "stereo": (2048, 512, 12.0, 3.0, None, "noise", True, 4),
}
SELECTION = (0.1, 0.45)        # seconds of nr_signal
STEREO_SHIFT = 1789            # samples: the second channel is nr_signal delayed (circularly) by this much


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    ref_gui.import_reference_gui(a.ref)
    import renoiser_gui as R
    from util import fourier, io_ops
    from util.fourier import to_mag
    from util.units import to_dB

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
    noise, noise_sr, _ = our_io.read_file(os.path.join(GOLDEN, "nr_noise.wav"))
    assert noise_sr == sr
    sig = sig if sig.ndim == 2 else sig[:, None]
    noise = noise if noise.ndim == 2 else noise[:, None]
    files = {"noise.wav": noise}
    written = {}
    io_ops.read_file = lambda path: (np.array(files[path], dtype=np.float32), sr, files[path].shape[1])
    io_ops.write_file = lambda path, data, rate, ch, suffix="_out": written.update(data=np.array(data), suffix=suffix, path=path, ch=ch)

    def resample_identity(x, sr_orig, sr_new, **kw):
        assert sr_orig == sr_new and kw.get("filter") == "sinc_window", (sr_orig, sr_new, kw)
        return x
    R.resampy.resample = resample_identity
    R.QtWidgets.QFileDialog.getOpenFileName = staticmethod(lambda *a, **k: ("noise.wav", ""))
    R.os = types.SimpleNamespace(path=types.SimpleNamespace(isfile=lambda p: p in files))

    def canvas(signal, fft, hop, gain, overhead, curve, channels):
        NS = ref_gui.NS
        anything = ref_gui._Anything()
        noise_widget = NS(gain=gain, overhead=overhead)
        parent = NS(curve=[list(p) for p in curve], line_control=anything, ax2=anything, line_noise=anything, line_final=anything,
                    ax=anything, mpl_canvas=anything, search_text_changed=lambda: None, props=NS(noise_widget=noise_widget, sel_str=""),
                    cfg={"dir_in": ""})
        spec = NS(audio_path="in.wav", signal=signal, selected_channel=0, fft_storage={}, key=None)
        c = NS(parent=parent, fft_size=fft, hop=hop, sr=sr, zeropad=1, spectra=[spec], filenames=["in.wav"],
               freqs=fourier.fft_freqs(fft, sr),
               props=NS(files_widget=NS(files=[NS(channel_widget=NS(channels=channels))])))
        c.noise_profile = np.full(len(c.freqs), -100.0, dtype=np.float32)
        c.final_profile = c.noise_profile.copy()
        c.px_to_spectrum = lambda click: click
        ref_gui._bind(c, R.Canvas, "redraw_plot", "get_mask_fac", "run_resample", "load_noise_profile", "on_mouse_release")
        return c

    out = {"sr": np.array(sr), "signal_sum": np.array(float(np.sum(sig, dtype=np.float64))),
           "noise_sum": np.array(float(np.sum(noise, dtype=np.float64))), "selection": np.array(SELECTION),
           "stereo_shift": np.array(STEREO_SHIFT), "near_db": np.array(NEAR_DB), "settings": np.array(sorted(SETTINGS))}
    for name, (fft, hop, gain, overhead, curve, source, stereo, stride) in SETTINGS.items():
        signal = np.concatenate([sig, np.roll(sig, STEREO_SHIFT, axis=0)], axis=1) if stereo else sig
        channels = [0, 1] if stereo else [0]
        c = canvas(signal, fft, hop, gain, overhead, curve if curve is not None else [[1, 0], [sr / 2, 0]], channels)
        with np.errstate(all="ignore"):
            if source == "noise":
                c.load_noise_profile()
            elif source == "select":
                c.spectra[0].key = (fft, 0, hop, 1)
                c.spectra[0].fft_storage[c.spectra[0].key] = fourier.get_mag(signal[:, 0], fft, hop, "blackmanharris", zeropad=1)
                t0, t1 = SELECTION
                event = types.SimpleNamespace(trail=lambda: [(t0, 0.0), (t1, 0.0)], button=1, modifiers=("Control",))
                c.on_mouse_release(event)
            else:
                c.redraw_plot()
            written.clear()
            c.run_resample()
            # the mask run_resample multiplied in, from the same STFT of the same padded channel
            n = len(signal)
            pad = fourier.fix_length(signal, n + fft // 2, axis=0)
            masks, near = [], []
            for ch in channels:
                S = np.array(fourier.stft(pad[:, ch], n_fft=fft, step=hop))
                fac = c.get_mask_fac(to_mag(S))
                masks.append(np.packbits((fac == 1.0).T.reshape(-1)))
                db = np.asarray(to_dB(to_mag(S)))
                f_i, b_i = np.nonzero(np.abs(db.T.astype(np.float64) - c.final_profile[None, :]) < NEAR_DB)
                near.append(np.stack([np.full(len(f_i), ch), f_i, b_i]).T)
                out[f"{name}_near_db_{ch}"] = db.T[f_i, b_i].astype(np.float32)
                out[f"{name}_frames"] = np.array(S.shape[1])
        y = written["data"]
        assert written["suffix"] == f" fft={fft}" and y.dtype == np.float32 and y.shape == (n, len(channels)), written["suffix"]
        out[f"{name}_params"] = np.array([fft, hop, gain, overhead, stride], dtype=np.float64)
        out[f"{name}_curve"] = np.array(curve if curve is not None else [[1, 0], [sr / 2, 0]], dtype=np.float64)
        out[f"{name}_noise_profile"] = np.asarray(c.noise_profile)          # float32 or float64, as the reference made it
        out[f"{name}_final"] = np.asarray(c.final_profile, dtype=np.float64)
        out[f"{name}_mask"] = np.stack(masks)
        out[f"{name}_near"] = np.concatenate(near).astype(np.int32)
        out[f"{name}_y"] = y[::stride].copy()
        out[f"{name}_peak"] = np.array(float(np.max(np.abs(y))))
        print(f"{name}: pass {np.mean(np.unpackbits(out[f'{name}_mask'][0]))[()]:.3f}, near {len(out[f'{name}_near'])}, "
              f"changed by {np.max(np.abs(y - signal[:, :len(channels)])) / np.max(np.abs(signal)):.3e} of the peak")
    out["backend"] = np.array(sorted(set(used)))
    save("renoiser", **out)


if __name__ == "__main__":
    main()
