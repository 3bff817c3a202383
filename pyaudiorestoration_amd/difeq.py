"""The Differential EQ tool of the reference (difeq_gui.py) on the GPU, headless.

    freqs, eq = get_eq("transfer.wav", "reference.wav", "L+R")        # difeq_gui.get_eq: reference minus source, dB per bin
    freqs_av, av = eq_curve(freqs, [eq], smoothing=50)                # the numeric part of MainWindow.plot
    export("eq", freqs_av, av)                                        # MainWindow.write: eq.txt, eq_L.txt, eq_R.txt for Audacity
    process([("a.wav", "a_ref.wav"), ("b.wav", "b_ref.wav")], "eq.txt")   # "Add EQ" for every pair, then "Export EQ"

get_eq is the whole cost of the tool: the time-averaged dB spectrum of two whole files at 16384 points.  Every file goes to the
device once and all its channels are averaged in one launch straight from the samples (par_stft_mean_db_f32, no spectrogram);
FUSED = False takes the chunked spectrogram path of spectrum_flat instead.  The spectra (8193 values per channel) come back to
the host, where the curve shaping and the export are the reference's numpy arithmetic, restated with its quirks.  There is no
CPU path for the spectra."""
import logging

import numpy as np
import torch

from . import _dev, fourier, io_ops, spectrum_flat

# True: the spectra come straight from the samples (par_stft_mean_db_f32) wherever the size allows; False: always through stored
# magnitude spectrograms in chunks (spectrum_flat.mean_spectrum_db_dev).  Measured (tools/bench_difeq.py, NOTES.md "Differential
# EQ"): stereo at 16384 / 8192, 10 min at 44.1 kHz 0.41 ms fused against 1.18 ms composed, 60 min at 192 kHz 8.4 against 29.3 ms, the
# results within 1.4e-13 dB of each other -- fused is the default.
FUSED = True
FFT_SIZE = 16384                            # difeq_gui.py:27-28
HOP = 8192
NUM_IN = 2000                               # difeq_gui.py:221
HEADER = 'FilterCurve: FilterLength="8191" InterpolateLin="0" InterpolationMethod="B-spline" '


def spectra_stereo(filename, fft_size=FFT_SIZE, hop=HOP, channel_mode="L+R", fused=None, device=None):
    """spectrum_flat.spectrum_from_audio_stereo(filename, fft_size, hop, channel_mode) with the file on the device once and its
    channels in one launch: -> ([float64 (bins,)] * 2, sr).  A mode that asks for the second channel of a mono file falls back to
    the first ("L+R") as the reference does; "R" on a mono file raises ValueError naming the file (the reference leaves its
    channel loop with an empty list there and dies with an IndexError)."""
    signal, sr, num_channels = io_ops.read_file(filename)
    dev = _dev.device_index(device)
    sig2d = signal if signal.ndim == 2 else signal[:, None]
    channels = []
    for channel in spectrum_flat.channel_map[channel_mode]:
        if channel == num_channels:
            logging.warning("not enough channels for L/R comparison  - fallback to mono")
            break
        channels.append(channel)
    if not channels:
        raise ValueError(f"{filename}: channel mode {channel_mode!r} needs a second channel, the file has {num_channels}")
    sig_t = _dev.to_dev(sig2d, torch.float32, dev)
    mean = spectrum_flat.mean_spectra_db_dev(sig_t, fft_size, hop, channels, "hann", fused=FUSED if fused is None else fused, dev=dev)
    spectra = list(_dev.to_host(mean))
    if channel_mode == "Mean":
        spectra = [np.mean(spectra, axis=0), ]
    if len(spectra) < 2:
        spectra.append(spectra[0])
    return spectra, sr


def get_eq(file_src, file_ref, channel_mode, fft_size=FFT_SIZE, hop=HOP, fused=None, device=None):
    """difeq_gui.get_eq (:24-38): -> (freqs (bins,), eq (2, bins) float64) = the reference file's time-averaged dB spectrum minus
    the source's, per channel (a mono file's only spectrum is used twice).  When the sample rates differ the reference's spectrum
    is put on the source's frequency grid with np.interp in host float64, as the reference does.  "R" on a mono file raises
    ValueError naming the file, where the reference dies with an IndexError."""
    spectra_src, sr_src = spectra_stereo(file_src, fft_size, hop, channel_mode, fused, device)
    spectra_ref, sr_ref = spectra_stereo(file_ref, fft_size, hop, channel_mode, fused, device)
    freqs = fourier.fft_freqs(fft_size, sr_src)
    if sr_src != sr_ref:
        freqs_ref = fourier.fft_freqs(fft_size, sr_ref)
        spectra_ref = [np.interp(freqs, freqs_ref, spectrum) for spectrum in spectra_ref]
    return freqs, np.asarray(spectra_ref) - np.asarray(spectra_src)


def _box_mean(a, n):
    """util/filters.py:27-30 to the bit: running sums, the sum n places back taken off from place n on, divided by n"""
    sums = np.cumsum(a, dtype=float)
    sums[n:] = sums[n:] - sums[:-n]
    return sums[n - 1:] / n


def eq_curve(freqs, eqs, highpass=0, rolloff_start=21000, rolloff_end=22000, resolution=200, smoothing=50, strength=100,
             keep_gain=False, return_gain=False):
    """The numeric part of MainWindow.plot (difeq_gui.py:212-257) on the list `eqs` of (2, bins) arrays get_eq returned:
    -> (freqs_av (k,), av (2, k)), with return_gain also the gain between the keys nearest 70 Hz and rolloff_end.
    The parameters are the spin boxes' integers (strength in percent).  Quirks kept: the mean over the EQs is interpolated onto
    np.power(2, linspace(log2 20, log2 freqs[-1], 2000)); curve and grid are box-averaged over `smoothing` points (which shortens
    them by smoothing - 1) and thinned with the step 2000 // resolution; the gain is taken off the curve for keep_gain (so that
    the EQ leaves the overall level alone); both fades multiply the curve, the high-pass one through np.interp with xp = (0, highpass),
    which for highpass = 0 is 1 everywhere but at a key of exactly 0 Hz."""
    freqs = np.asarray(freqs)
    step = NUM_IN // resolution
    av_in = np.mean(np.asarray(eqs), axis=0)
    freqs_spaced = np.power(2, np.linspace(np.log2(20), np.log2(freqs[-1]), num=NUM_IN))
    freqs_av = _box_mean(freqs_spaced, smoothing)[::step]
    av = np.asarray([_box_mean(np.interp(freqs_spaced, freqs, av_in[channel]), smoothing)[::step] for channel in (0, 1)])
    idx1 = np.abs(freqs_av - 70).argmin()
    idx2 = np.abs(freqs_av - rolloff_end).argmin()
    gain = np.mean(av[:, idx1:idx2])
    if keep_gain:
        av -= gain
    av *= strength / 100
    for channel in (0, 1):
        av[channel] *= np.interp(freqs_av, (rolloff_start, rolloff_end), (1, 0))
        av[channel] *= np.interp(freqs_av, (0, highpass), (0, 1))
    return (freqs_av, av, gain) if return_gain else (freqs_av, av)


def write_eq_txt(path, freqs, dB):
    """difeq_gui.write_eq_txt (:16-21): Audacity's FilterCurve preset line, keys f<i>="..." v<i>="..." in Python's repr of the
    float64 values"""
    with open(path, "w") as out:
        out.write(HEADER)
        for i, (f, d) in enumerate(zip(freqs, dB)):
            out.write(f'f{i}="{f}" v{i}="{d}" ')


def export(base, freqs_av, av):
    """MainWindow.write (difeq_gui.py:197-206): <base>.txt holds the mean of the two channels, <base>_L.txt and <base>_R.txt the
    channels -> the three paths"""
    paths = [f"{base}.txt", f"{base}_L.txt", f"{base}_R.txt"]
    write_eq_txt(paths[0], freqs_av, np.mean(av, axis=0))
    write_eq_txt(paths[1], freqs_av, av[0])
    write_eq_txt(paths[2], freqs_av, av[1])
    return paths


def process(pairs, out, channel_mode="L+R", device=None, **curve_params):
    """"Add EQ" for every (source, reference) pair of `pairs`, then "Export EQ" to `out` (eq.txt -> eq.txt, eq_L.txt, eq_R.txt;
    the text behind the last dot is dropped as MainWindow.write does).  The frequency grid is the last pair's, as in the GUI.
    curve_params: eq_curve's.  -> {"paths", "freqs_av", "av", "gain", "eqs"}"""
    _dev.device_index(device)                       # no GPU: stop before touching a file
    if not pairs:
        raise ValueError("no (source, reference) pair")
    base = ".".join(out.split(".")[:-1])
    if not base:
        raise ValueError(f"{out!r}: the output needs a name and an extension, like eq.txt")
    eqs, freqs = [], None
    for file_src, file_ref in pairs:
        freqs, eq = get_eq(file_src, file_ref, channel_mode, device=device)
        eqs.append(eq)
    freqs_av, av, gain = eq_curve(freqs, eqs, return_gain=True, **curve_params)
    return {"paths": export(base, freqs_av, av), "freqs_av": freqs_av, "av": av, "gain": gain, "eqs": eqs}
