"""Cyclic wow analysis of the reference (experiments/cyclic_wow.py) on the GPU, headless: the wow of an off-centre or warped record
measured from a pilot tone.

    res = analyse("side_a.wav", rpm=33.333, pilot_hz=3150.0)          # the script as a whole
    res.frames_per_rotation, res.cycle_duration, res.rpm_measured, res.delta      # delta in octaves
    curve = speed_curve(res, sr, hop)                                   # [[t, speed], ...] for resampling.run(speed_curve=...)

The script takes a dB spectrogram at 16384 points and a hop of 128 samples (every sample transformed 128 times), runs PeakTracker
along a constant trail and folds log2 of the track at every cycle length within 10 % of the nominal rotation.  Here the track comes
straight from the samples (par_stft_track_peak_f64: one float64 per frame leaves the transform kernel, no spectrogram is stored)
and all candidate lengths are folded in one launch (par_cycle_fold_f64).  FUSED = False composes the parent kernels instead: K_stft
mode 1 in chunks of bounded bytes and par_track_peak_f64 per chunk.  The file goes to the device once; the track, the table of
candidates and the best fold come back.  There is no CPU path."""
import collections

import numpy as np
import torch

from . import _dev, _lib, fourier, io_ops, spectrum_flat
from .wow_detection import interp_nans, sample_trail

# True: the track comes straight from the samples (par_stft_track_peak_f64) wherever the size allows; False: always through stored
# magnitude spectrograms in chunks.  Measured (tools/bench_cyclic.py, NOTES.md "Cyclic wow"): 16384 / 128, 1 min at 44.1 kHz 0.71 ms
# fused against 3.35 ms composed, 20 min 12.0 against 62.7 ms, the spread of the composed medians 0.02 / 0.22 ms, the two tracks
# bit-identical -- fused is the default.
FUSED = True
FFT_SIZE = 16384                            # experiments/cyclic_wow.py:32-33
OVERLAP = 128
MODES = {"Peak": 0, "Peak Track": 1}

CyclicWow = collections.namedtuple("CyclicWow", "frames_per_rotation delta cycle_duration rpm_measured avg results times freqs")


def fused_supported(fft_size, zeropad=1):
    """Sizes par_stft_track_peak_f64 takes: n_fft * zeropad a power of two in [16, 16384]"""
    return spectrum_flat.fused_mean_supported(fft_size, zeropad)


def default_hop(fft_size):
    """fft_size // 128 (experiments/cyclic_wow.py:33)"""
    return int(fft_size) // OVERLAP


def candidate_range(frames_init, tolerance=0.1):
    """-> (first candidate, number of candidates, d): d = int(frames_init * tolerance), candidates frames_init - d ..
    frames_init + d - 1 (experiments/cyclic_wow.py:50-54)"""
    d = int(frames_init * tolerance)
    return int(frames_init) - d, 2 * d, d


def channel_index(channel, num_channels):
    """"L" / "R" (spectrum_flat.channel_map) or a channel number -> index; a channel the signal does not have is a ValueError"""
    ch = spectrum_flat.channel_map[channel][0] if isinstance(channel, str) else int(channel)
    if not 0 <= ch < num_channels:
        raise ValueError(f"channel {channel!r} of a {num_channels}-channel signal")
    return ch


def _channel_dev(signal, channel, dev):
    """numpy or device signal, (n,) or (n, ch) -> (1-D float32 device view of the channel, element stride, n)"""
    if isinstance(signal, torch.Tensor):
        sig_t = signal if signal.is_cuda and signal.dtype == torch.float32 else _dev.to_dev(signal, torch.float32, dev)
    else:
        sig_t = _dev.to_dev(np.asarray(signal), torch.float32, dev)
    if sig_t.ndim == 1:
        sig_t = sig_t[:, None]
    if sig_t.ndim != 2 or not 0 <= channel < sig_t.shape[1]:
        raise ValueError(f"channel {channel} of a signal of shape {tuple(sig_t.shape)}")
    n = sig_t.shape[0]
    x_t = sig_t[:, channel]
    return x_t, (x_t.stride(0) if n > 1 else 1), n


def pilot_track(signal, sr, trail, fft_size=FFT_SIZE, hop=None, tolerance_st=10, channel=0, db=True, mode="Peak", window="hann",
                zeropad=1, fused=None, device=None, chunk_bytes=spectrum_flat.CHUNK_BYTES):
    """The spectrogram and tracker of experiments/cyclic_wow.py:34-48 -> (times, freqs, frame_0, frame_1): what PeakTracker
    (mode "Peak") or PeakTrackTracker ("Peak Track") leaves in .times / .freqs on the spectrogram of one channel of `signal`
    (numpy or device tensor, (n,) or (n, channels)) along `trail` [(t seconds, f Hz), ...], tolerance in semitones.  db: the tracker
    reads float32 dB (the script's to_dB spectrogram) instead of the magnitudes pyrespeeder's trackers read.  hop=None is
    fft_size // 128.  fused (default FUSED): par_stft_track_peak_f64, no spectrogram stored; otherwise, and above 16384 points,
    K_stft mode 1 in chunks of at most chunk_bytes, the dB taken on the device, par_track_peak_f64 per chunk ("Peak Track" then
    needs its span inside one chunk: its band hangs on the first frame).  The reference's errors keep their types: an empty band
    is a ValueError (ParEmptyBand), a peak on the last bin an IndexError (ParIndexError), a band past the last bin a ValueError
    (ParShapeError)."""
    dev = _dev.device_index(device if device is not None else (signal.device if isinstance(signal, torch.Tensor) and signal.is_cuda else None))
    if mode not in MODES:
        raise ValueError(f"mode {mode!r}: one of {sorted(MODES)}")
    fft_size, zeropad = int(fft_size), int(zeropad)
    hop = default_hop(fft_size) if hop is None else int(hop)
    x_t, stride, n = _channel_dev(signal, int(channel), dev)
    L = _lib.lib()
    n_frames = int(L.par_stft_frames(n, fft_size, hop))
    frame_0, frame_1, times, freqs = sample_trail(trail, n_frames, hop, sr)
    count = len(freqs)
    if count == 0:
        if MODES[mode] == 1:
            raise IndexError("index 0 is out of bounds for axis 0 with size 0")
        return times, freqs, frame_0, frame_1
    window_t = fourier.window_dev(window, fft_size, dev)
    f_t = _dev.to_dev(freqs, torch.float64, dev)
    status = _dev.empty(1, torch.int32, dev)
    tol = float(tolerance_st / 12)                          # semitones -> octaves
    if (FUSED if fused is None else fused) and fused_supported(fft_size, zeropad):
        _lib.check(L.par_stft_track_peak_f64(dev, _dev.ptr(x_t), n, stride, fft_size, hop, zeropad, _dev.ptr(window_t), frame_0, count,
                                             _dev.ptr(f_t), float(sr), tol, MODES[mode], 1 if db else 0, _dev.ptr(status),
                                             _dev.stream_ptr(dev)))
    else:
        bins = fft_size * zeropad // 2 + 1
        for f0, f1, fm in spectrum_flat.mag_chunks_dev(x_t, fft_size, hop, window_t, zeropad, stride, n, dev, chunk_bytes):
            lo, hi = max(f0, frame_0), min(f1, frame_1)
            if lo >= hi:
                continue
            if MODES[mode] == 1 and lo != frame_0:
                raise ValueError("Peak Track composes inside one spectrogram chunk only: raise chunk_bytes or take the fused path")
            if db:                                          # (float)(20 log10((double) m)), row block by row block
                for r0 in range(lo - f0, hi - f0, 4096):
                    rows = fm[r0:min(r0 + 4096, hi - f0), :bins]
                    rows.copy_((20.0 * torch.log10(rows.to(torch.float64))).to(torch.float32))
            _lib.check(L.par_track_peak_f64(dev, _dev.ptr(fm), f1 - f0, bins, fm.stride(0), lo - f0, hi - lo,
                                            _dev.ptr(f_t[lo - frame_0:]), fft_size * zeropad, float(sr), tol, MODES[mode],
                                            _dev.ptr(status), _dev.stream_ptr(dev)))
    freqs[:] = f_t.cpu().numpy()
    interp_nans(freqs)
    return times, freqs, frame_0, frame_1


def _fold_dev(logfreq, p_first, n_cand, want_avg, dev):
    dev = _dev.device_index(dev if dev is not None else (logfreq.device if isinstance(logfreq, torch.Tensor) and logfreq.is_cuda else None))
    v_t = _dev.to_dev(logfreq, torch.float64, dev).reshape(-1)
    p_first, n_cand = int(p_first), int(n_cand)
    pitch = max(p_first + n_cand - 1, 1)
    avg = _dev.empty((max(n_cand, 1), pitch), torch.float64, dev) if want_avg else None
    delta = _dev.empty(max(n_cand, 1), torch.float64, dev)
    _lib.check(_lib.lib().par_cycle_fold_f64(dev, _dev.ptr(v_t), v_t.numel(), p_first, n_cand, _dev.ptr(avg) if want_avg else None,
                                             pitch, _dev.ptr(delta), _dev.stream_ptr(dev)))
    return avg, delta


def fold(logfreq, frames_per_rotation, device=None):
    """get_avg (experiments/cyclic_wow.py:9-27): the track cut into len // frames_per_rotation whole views and averaged over them,
    np.mean(np.split(logfreq[:views * frames_per_rotation], views), axis=0) -> float64 (frames_per_rotation,): the views added one
    after the other from the first, then one division, which is numpy's order and its bits for every length but 1 (there numpy
    sums the single column pairwise)."""
    avg, _ = _fold_dev(logfreq, frames_per_rotation, 1, True, device)
    return avg[0].cpu().numpy()


def cycle_search(logfreq, frames_init, tolerance=0.1, device=None):
    """The search loop (experiments/cyclic_wow.py:50-59) -> results (2 d, 2) float64, d = int(frames_init * tolerance): row k holds
    the candidate cycle length frames_init - d + k and the max - min of the track folded at it.  All candidates in one launch."""
    p_first, n_cand, d = candidate_range(frames_init, tolerance)
    results = np.empty((d * 2, 2))
    if d < 1:
        return results
    _, delta = _fold_dev(logfreq, p_first, n_cand, False, device)
    results[:, 0] = np.arange(p_first, p_first + n_cand)
    results[:, 1] = delta.cpu().numpy()
    return results


def best_cycle(results):
    """np.argmax over the deltas, first occurrence (experiments/cyclic_wow.py:63-64) -> (frames_per_rotation, delta)"""
    frames_per_rotation, delta = results[np.argmax(results[:, 1])]
    return int(frames_per_rotation), float(delta)


def analyse(path_or_signal, sr=None, rpm=45.0, pilot_hz=700.0, tolerance=0.1, tolerance_st=10, fft_size=FFT_SIZE, hop=None,
            channel="L", fused=None, db=True, device=None):
    """experiments/cyclic_wow.py as a whole on a file (or on a signal with its sample rate) -> CyclicWow(frames_per_rotation, delta,
    cycle_duration, rpm_measured, avg, results, times, freqs).  The pilot is traced along a constant trail over the whole file,
    log2 of the track is folded at every cycle length within `tolerance` of the nominal rotation at `rpm`, the length whose fold
    has the largest max - min wins.  delta is in octaves (delta * 12 semitones; the script prints delta / 12 and calls it
    semitones), cycle_duration in seconds, avg the winning fold (log2 Hz per frame of the cycle)."""
    dev = _dev.device_index(device)
    if isinstance(path_or_signal, str):
        signal, sr, _ = io_ops.read_file(path_or_signal)
    else:
        signal = path_or_signal
        if sr is None:
            raise ValueError("a signal needs its sample rate")
    fft_size = int(fft_size)
    hop = default_hop(fft_size) if hop is None else int(hop)
    n = signal.shape[0]
    ch = channel_index(channel, 1 if signal.ndim == 1 else signal.shape[1])
    trail = [(0.0, float(pilot_hz)), (n / sr, float(pilot_hz))]
    times, freqs, _, _ = pilot_track(signal, sr, trail, fft_size, hop, tolerance_st, ch, db, "Peak", fused=fused, device=dev)
    logfreq = np.log2(freqs)
    frames_init = int(60.0 / rpm * sr / hop)                # experiments/cyclic_wow.py:40-45
    logf_t = _dev.to_dev(logfreq, torch.float64, dev)
    results = cycle_search(logf_t, frames_init, tolerance, dev)
    frames_per_rotation, delta = best_cycle(results)
    avg = fold(logf_t, frames_per_rotation, dev)
    cycle_duration = frames_per_rotation * hop / sr
    return CyclicWow(frames_per_rotation, delta, cycle_duration, 60.0 / cycle_duration, avg, results, times, freqs)


def speed_curve(result, sr, hop):
    """An extension of this port (the script stops at the plot): the measured cycle tiled over the file, in the shape
    pipeline.master_speed_curve(lines, duration, sr, hop) returns -- [[t seconds, linear speed], ...] with speed
    2 ** (avg[i % P] - mean(avg)) at result.times[i], the tracker's own time grid -- which is what
    resampling.run(speed_curve=...) takes to remove the cycle.  sr and hop only check that the grid is the one of that analysis."""
    avg = np.asarray(result.avg, dtype=np.float64)
    t = np.asarray(result.times, dtype=np.float64)
    if len(t) > 1 and abs((t[1] - t[0]) * sr / hop - 1.0) > 0.01:
        raise ValueError(f"the track's frames are {t[1] - t[0]} s apart, not {hop} samples at {sr} Hz")
    return np.stack((t, np.power(2.0, avg[np.arange(len(t)) % len(avg)] - np.mean(avg))), axis=-1)


def report(result):
    """The figures the script prints, as a dict (delta in octaves and in semitones)"""
    return {"frames_per_rotation": int(result.frames_per_rotation), "cycle_duration_s": float(result.cycle_duration),
            "rpm_measured": float(result.rpm_measured), "delta_octaves": float(result.delta), "delta_semitones": float(result.delta) * 12.0}
