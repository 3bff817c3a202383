"""Headless restatement of the hum speed analysis tool (reference humspeed_gui.py): find the mains hum and its harmonics in the
long-time averaged spectrum of a recording, read off how far they are from their nominal frequencies, and resample the file by
that ratio.

    freqs, spectrum, sr = get_spectrum("tape.wav", "L+R")          # get_spectrum (humspeed_gui.py:18-24), 2^19-point frames
    res = analyse("tape.wav", base_hum=50, num_harmonies=2)        # update_spectrum + on_hum_param_changed (:100-126)
    resample_file("tape.wav", res["ratios"][-1])                   # resample (:185-198) -> tape_resampled_<percent>.wav

The averaged spectrum is spectrum_flat.spectrum_from_audio (K_stft's four-step transform and the chunked dB mean, hop = twice
the frame); the peak search is the reference's host arithmetic (two argmins, an argmax over the slice, correlation.parabolic);
the resampling is fixed_rate.resample (K_rsfix) where the reference calls resampy."""
import logging
import os

import numpy as np

from . import correlation, fixed_rate, fourier, io_ops, spectrum_flat

FFT_SIZE = 524288  # 2**19, the GUI's fixed size


def get_spectrum(file_src, channel_mode, fft_size=FFT_SIZE):
    """-> (freqs, spectrum, sr): the time-averaged dB spectrum of the file's selected channels, hop = 2 * fft_size."""
    logging.info(f"Analyzing channels: {channel_mode}")
    hop = fft_size * 2
    spectrum, sr = spectrum_flat.spectrum_from_audio(file_src, fft_size, hop, channel_mode)
    freqs = fourier.fft_freqs(fft_size, sr)
    return freqs, spectrum, sr


def hum_freqs(base_hum=50, num_harmonies=2):
    """The hum and its harmonics the GUI looks for (on_hum_param_changed)."""
    return np.arange(base_hum, base_hum + base_hum * num_harmonies + 1, base_hum)


def track_to(freqs, spectrum, sr, fft_size, xpos, hum_freqs, tolerance=8):
    """MainWindow.track_to around the frequency xpos: the highest bin within +-tolerance percent, refined by a parabola ->
    (freq, dB, ratio) with ratio = nearest hum frequency / freq, or None when that is more than tolerance percent off ("hum was
    not close enough")."""
    l_ratio = 1 - tolerance / 100
    r_ratio = 1 + tolerance / 100
    border_L = max(np.argmin(np.abs(freqs - xpos * l_ratio)), 0)
    border_R = min(np.argmin(np.abs(freqs - xpos * r_ratio)), len(freqs))
    raw_index = np.argmax(spectrum[border_L:border_R]) + border_L
    interp_index, dB = correlation.parabolic(spectrum, raw_index)
    freq = interp_index * sr / fft_size
    closest_hum = hum_freqs[np.argmin(np.abs(hum_freqs - freq))]
    ratio = closest_hum / freq
    percent = (ratio - 1) * 100
    if abs(percent) > tolerance:
        logging.info("hum was not close enough")
        return None
    return freq, dB, ratio


def analyse(file_src, channel_mode="L+R", base_hum=50, num_harmonies=2, tolerance=8, fft_size=FFT_SIZE):
    """update_spectrum + on_hum_param_changed: the markers of every hum frequency that was found, in the reference's order ->
    {"freqs", "spectrum", "sr", "hum_freqs", "marker_freqs", "marker_dBs", "ratios"}.  The GUI's Resample button uses
    ratios[-1]."""
    freqs, spectrum, sr = get_spectrum(file_src, channel_mode, fft_size)
    hums = hum_freqs(base_hum, num_harmonies)
    marker_freqs, marker_dBs, ratios = [], [], []
    for hum in hums:
        found = track_to(freqs, spectrum, sr, fft_size, hum, hums, tolerance)
        if found is not None:
            marker_freqs.append(found[0])
            marker_dBs.append(found[1])
            ratios.append(found[2])
            logging.debug("hum %g Hz found at %.4f Hz (%.2f dB): Percent Change: %.3f", hum, found[0], found[1], (found[2] - 1) * 100)
    return {"freqs": freqs, "spectrum": spectrum, "sr": sr, "hum_freqs": hums, "marker_freqs": marker_freqs,
            "marker_dBs": marker_dBs, "ratios": ratios}


def resampled_suffix(ratio):
    return "_resampled_%.3f" % ((ratio - 1) * 100)


def resample_file(path, ratio, device=None, signal_data=None):
    """MainWindow.resample: the whole file resampled from sr * ratio to sr and written as "<stem>_resampled_<percent>.wav"
    (signal_data=(signal, sr, channels) skips the read).  Returns the written path."""
    logging.info("Resampling")
    signal, sr, num_channels = io_ops.read_file(path) if signal_data is None else signal_data
    res = fixed_rate.resample(signal, sr * ratio, sr, axis=0, filter='sinc_window', num_zeros=8, device=device)
    suffix = resampled_suffix(ratio)
    io_ops.write_file(path, res, sr, num_channels, suffix)
    return f"{os.path.splitext(path)[0]}{suffix}.wav"
