"""Headless restatement of the renoiser, the suite's noise-floor tool (reference renoiser_gui.Canvas; experiments/renoiser.py is
its command-line prototype).

    prof = noise_profile(noise, noise_sr, sr)                     # load_noise_profile (renoiser_gui.py:239-250)
    prof = noise_profile_from_selection(signal, sr, t0, t1)       # on_mouse_release (:327-345)
    final = final_profile(prof, sr, 2048)                         # redraw_plot (:280-294)
    out = renoise(signal, sr, final)                              # get_mask_fac + run_resample (:273-278, :296-319)
    renoise_file("tape.wav", noise_path="hiss.wav")               # ... written as "tape fft=2048.wav"
    offsets, stds, pad = sniff_offset(signal, sr)                 # sniff_offset, "Gauge offset" (:347-369)
    out = renoise_offset(signal, sr, final, pad)                  # ... and its use (experiments/renoiser.py:60-65)

Per selected channel the reference zero-extends the signal by n_fft/2, takes a complex STFT (blackmanharris, zero padding 1),
multiplies a binary per-bin gain mask in (a bin whose float32 dB is above the final profile passes, every other bin gets `gain`
dB) and runs the ISTFT.  Here that whole chain is one launch of par_gate_stft_f32 for all channels (n_fft <= 8192: no
spectrogram reaches HBM); larger transforms compose K_stft, par_gate_spectrum_f32 and K_istft.  The mask's float32 decibels
become one float32 magnitude cutoff per bin on the host (gate_cutoffs), so the kernels decide exactly as numpy does on the
same spectrum.

"Gauge offset" looks for the frame alignment of an earlier frame-wise denoise: for every pad i < hop the reference puts i zeros
in front of channel 0, zero-extends by n_fft/2, takes a whole complex STFT, averages bins 3-12 kHz per frame and takes the
standard deviation of that series; the best pad is the argmax.  The band mean of a windowed frame is its inner product with one
complex vector (gauge_filter), so the hop transforms become one n_fft-tap complex FIR over the signal, sorted into hop residue
classes (par_gauge_offset_f32: no FFT, no spectrogram).  renoise_offset(..., offset=k) (renoise_dev and renoise_file take the
same argument) applies the gate with k zeros in front of every selected channel and drops them from the result; renoise keeps
its parameter list.

Differences from the reference:
- gauge_band raises ValueError for a band that holds no bin (the reference would average nothing and return NaN).
- Noise at another sample rate raises ValueError unless resample_noise=True asks for the GUI's pass through the sinc_window
  resampler (num_zeros=8), which is fixed_rate.resample here (float32 sums, resampy computes in the file's dtype); the profile
  is taken from the samples as given when the rates are equal, which is also what experiments/renoiser.py does then.
- An empty selection (no frame between t0 and t1) raises ValueError; the reference would produce a NaN profile.
- The input is never modified.  Repeated channel numbers raise ValueError (the reference leaves the columns they skip
  uninitialised); a channel number at or above the number of selected channels raises IndexError, as the reference's
  y_out[:, channel_i] does.
- Both profiles are float64 sums over frames of the float32 magnitudes K_stft computes (decibels for a noise file); the
  reference's numpy backend averages float64 values of its own STFT.  NOTES.md gives the bound.
"""
import logging
import os

import numpy as np
import torch
from scipy import signal as dsp

from . import _dev, _lib, fixed_rate, fourier, io_ops, spectrum_flat

WINDOW = "blackmanharris"
# GUI defaults (util/widgets.py:768-810, 326-351): FFT 2048, overlap 4, gain 12 dB, overhead 3 dB, zero padding forced to 1
FFT_SIZE, OVERLAP, GAIN, OVERHEAD = 2048, 4, 12.0, 3.0
NO_PROFILE_DB = -100.0


def _as_2d(signal):
    return signal if signal.ndim == 2 else signal[:, None]


def _db32(mag):
    """util/units.to_dB on float32 magnitudes: float32 20 * log10(m)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(20) * np.log10(np.asarray(mag, dtype=np.float32))


def default_profile(sr, fft_size=FFT_SIZE):
    """The profile before any noise is loaded: -100 dB in every bin (renoiser_gui.py:204-205)."""
    return np.full(len(fourier.fft_freqs(fft_size, sr)), NO_PROFILE_DB, dtype=np.float32)


def noise_profile(noise, noise_sr, sr, fft_size=FFT_SIZE, hop=FFT_SIZE // OVERLAP, device=None, resample_noise=False):
    """Mean decibel spectrum of the first channel of a noise recording, float64 (bins,) like the reference's numpy STFT backend
    makes it -- load_noise_profile.  Noise at another rate than the signal's: ValueError by default; with resample_noise=True
    it is first resampled to the signal's rate, fixed_rate.resample(noise, noise_sr, sr), as the GUI does with resampy."""
    if int(noise_sr) != int(sr) and not resample_noise:
        raise ValueError(f"noise sample rate {noise_sr} != signal rate {sr}: resample the noise first (no resampy pass here; "
                         "resample_noise=True runs fixed_rate.resample)")
    dev = _dev.device_index(device if device is not None else (noise.device if torch.is_tensor(noise) else None))
    if int(noise_sr) != int(sr):
        # channels are independent and only the first is read below
        noise = fixed_rate.resample(_dev.to_dev(_as_2d(noise)[:, 0], torch.float32, dev), noise_sr, sr, axis=0,
                                    filter='sinc_window', num_zeros=8, device=dev)
    n2d = _as_2d(noise)
    n, ch = n2d.shape
    flat = _dev.to_dev(n2d, torch.float32, dev).reshape(-1)
    mean = spectrum_flat.mean_spectrum_db_dev(flat, fft_size, hop, WINDOW, 1, x_stride=ch, n=n, dev=dev)
    return _dev.to_host(mean)


def selection_frames(t0, t1, sr, hop, n_frames):
    """Frame range [f0, f1) of a selection from t0 to t1 seconds (renoiser_gui.py:336-341)."""
    f0 = max(0, int(t0 * sr / hop))
    f1 = min(int(t1 * sr / hop), n_frames - 1)
    return f0, f1


def noise_profile_from_selection(signal, sr, t0, t1, fft_size=FFT_SIZE, hop=FFT_SIZE // OVERLAP, channel=0, device=None):
    """to_dB of the mean magnitude spectrum (|X| + 1e-7) of frames [f0, f1) of one channel, float64 (bins,) --
    on_mouse_release.  ValueError when the range holds no frame."""
    s2d = _as_2d(signal)
    n, ch = s2d.shape
    if not 0 <= channel < ch:
        raise IndexError(f"channel {channel} of a {ch}-channel signal")
    frames = int(_lib.lib().par_stft_frames(n, fft_size, hop))
    f0, f1 = selection_frames(t0, t1, sr, hop, frames)
    if f1 <= f0:
        raise ValueError(f"the selection {t0}-{t1} s holds no frame (frames {f0}..{f1}): the reference would make a NaN profile")
    dev = _dev.device_index(device if device is not None else (signal.device if torch.is_tensor(signal) else None))
    flat = _dev.to_dev(s2d, torch.float32, dev).reshape(-1)
    window_t = fourier.window_dev(WINDOW, fft_size, dev)
    bins = fft_size // 2 + 1
    acc = torch.zeros(bins, dtype=torch.float64, device=f"cuda:{dev}")
    L = _lib.lib()
    for c0, c1, fm in spectrum_flat.mag_chunks_dev(flat[channel:], fft_size, hop, window_t, 1, ch, n, dev):
        a, b = max(c0, f0), min(c1, f1)
        if a < b:
            rows = fm[a - c0:b - c0]
            _lib.check(L.par_mean_mag_frames_f32(dev, _dev.ptr(rows), b - a, bins, rows.stride(0), _dev.ptr(acc), _dev.stream_ptr(dev)))
    return 20 * np.log10(_dev.to_host(acc) / (f1 - f0))


def final_profile(noise_profile, sr, fft_size=FFT_SIZE, gain=GAIN, overhead=OVERHEAD, curve=None):
    """noise profile + gain + the control curve interpolated at the bin frequencies + overhead, float64 (bins,) -- redraw_plot.
    curve: [[Hz, dB], ...] (default [[1, 0], [sr/2, 0]]), sorted like the GUI's list.  The profile keeps its dtype: for a
    float32 profile the gain is added in float32 first, exactly as numpy does there."""
    freqs = fourier.fft_freqs(fft_size, sr)
    pts = sorted([list(p) for p in ([[1, 0], [sr / 2, 0]] if curve is None else curve)])
    cx, cy = zip(*pts)
    prof = np.asarray(noise_profile)
    if prof.dtype not in (np.float32, np.float64):
        prof = prof.astype(np.float64)
    if prof.shape != freqs.shape:
        raise ValueError(f"noise profile has {prof.shape} bins, the FFT size {fft_size} has {freqs.shape}")
    return prof + float(gain) + np.interp(freqs, cx, cy) + float(overhead)


def gate_cutoffs(final):
    """float32 magnitude cutoffs of a float64 threshold profile: for every float32 magnitude m >= 0,
    float32(20 log10(m)) > final[k]  <=>  m >= cutoff[k]  (numpy's float32 log10 is monotone).  Found by bisection over the
    float32 bit patterns with numpy's own float32 decibels; a threshold no magnitude exceeds (NaN, +inf) gives a NaN cutoff,
    which gates every magnitude, NaN included."""
    thr = np.asarray(final, dtype=np.float64)

    def above(bits):
        return _db32(bits.view(np.float32)) > thr
    lo = np.zeros(thr.shape, dtype=np.uint32)                       # 0.0: -inf dB, above no threshold
    hi = np.full(thr.shape, 0x7F800000, dtype=np.uint32)            # +inf
    ok = above(hi.copy())
    while True:
        gap = hi - lo
        if not np.any(gap > 1):
            break
        mid = lo + gap // 2
        m_above = above(mid)
        hi = np.where(m_above, mid, hi)
        lo = np.where(m_above, lo, mid)
    cut = hi.view(np.float32).copy()
    cut[~ok] = np.nan
    return cut


def low_factor(gain):
    """The mask's factor for gated bins: float32(10^(gain/20)) (util/units.to_fac in float64, then float32)."""
    return np.float32(np.power(10, float(gain) / 20))


GAUGE_BAND = (3000, 12000)


def gauge_band(sr, fft_size, band=GAUGE_BAND):
    """Bins [l, u) the gauge averages: int(round(f * fft_size / sr)) for both ends (renoiser_gui.py:352-353), u clipped to the
    number of bins as the reference's slice clips it.  ValueError when the band holds no bin."""
    l = int(round(band[0] * fft_size / sr))
    u = min(int(round(band[1] * fft_size / sr)), fft_size // 2 + 1)
    if l < 0 or u <= l:
        raise ValueError(f"gauge band {band[0]}-{band[1]} Hz holds no bin of a {fft_size}-point transform at {sr} Hz "
                         f"(bins {l}..{u}): the reference would average nothing")
    return l, u


def gauge_filter(sr, fft_size, band=GAUGE_BAND):
    """complex128 (fft_size,): h[m] = w32[m] * sum_{k=l}^{u-1} exp(-2 pi i k m / N) / (sqrt(N) (u - l)), so that the mean of
    bins l..u-1 of the reference's STFT frame (float32 blackmanharris window, scaled by 1/sqrt(N)) is sum_m frame[m] h[m]."""
    n_fft = int(fft_size)
    l, u = gauge_band(sr, n_fft, band)
    w = dsp.get_window(WINDOW, n_fft).astype(np.float32).astype(np.float64)
    m = np.arange(n_fft, dtype=np.int64)
    acc = np.zeros(n_fft, dtype=np.complex128)
    for k0 in range(l, u, 256):                                      # (k m) mod N keeps the phase exact for any size
        k = np.arange(k0, min(u, k0 + 256), dtype=np.int64)
        acc += np.exp(-2j * np.pi * ((k[:, None] * m[None, :]) % n_fft) / n_fft).sum(axis=0)
    return w * acc / (np.sqrt(n_fft) * (u - l))


_gauge_filter_cache = {}


def gauge_filter_dev(sr, fft_size, band, dev):
    """gauge_filter rounded to float32 as a (2, fft_size) device tensor (real row, imaginary row), kept per (rate, size, band,
    device) like fourier.window_dev: the host sum and the upload cost more than the kernel."""
    key = (float(sr), int(fft_size), float(band[0]), float(band[1]), dev)
    h_t = _gauge_filter_cache.get(key)
    if h_t is None:
        if len(_gauge_filter_cache) > 64:
            _gauge_filter_cache.clear()
        h = gauge_filter(sr, fft_size, band)
        h_t = _gauge_filter_cache[key] = _dev.to_dev(np.stack((h.real, h.imag)).astype(np.float32), torch.float32, dev)
    return h_t


def sniff_offset_dev(sig_t, sr, fft_size=FFT_SIZE, hop=FFT_SIZE // OVERLAP, channel=0, band=GAUGE_BAND, dev=None, out=None):
    """Device form of sniff_offset: sig_t float32 (n, ch) or (n,) device tensor -> float64 (hop,) device tensor of the curve
    (out: a float64 tensor of at least hop cells to write it to, returned as it is).  One call of par_gauge_offset_f32."""
    fft_size, hop = int(fft_size), int(hop)
    if fft_size < 2 or hop < 1:
        raise ValueError(f"fft_size {fft_size} / hop {hop}: need fft_size >= 2 and hop >= 1")
    gauge_band(sr, fft_size, band)                                   # ValueError for an empty band, before any device work
    dev = _dev.device_index(dev if dev is not None else sig_t.device)
    h_t = gauge_filter_dev(sr, fft_size, band, dev)
    s2d = _as_2d(sig_t)
    n, ch = s2d.shape
    if not 0 <= channel < ch:
        raise IndexError(f"channel {channel} of a {ch}-channel signal")
    if n < 1:
        raise ValueError("empty signal")
    L = _lib.lib()
    flat = _dev.to_dev(s2d, torch.float32, dev).reshape(-1)
    nbytes = int(L.par_gauge_scratch_bytes(n, fft_size, hop))
    scratch = _dev.empty((nbytes + 7) // 8, torch.float64, dev)
    stds = _dev.empty(hop, torch.float64, dev) if out is None else out
    if stds.dtype != torch.float64 or stds.numel() < hop or not stds.is_contiguous():
        raise ValueError("out: a contiguous float64 tensor of at least hop cells")
    _lib.check(L.par_gauge_offset_f32(dev, _dev.ptr(flat[channel:]), n, ch, fft_size, hop, _dev.ptr(h_t[0]), _dev.ptr(h_t[1]),
                                      _dev.ptr(stds), _dev.ptr(scratch), scratch.numel() * 8, _dev.stream_ptr(dev)))
    return stds


def sniff_offset(signal, sr, fft_size=FFT_SIZE, hop=FFT_SIZE // OVERLAP, channel=0, band=GAUGE_BAND, device=None):
    """Canvas.sniff_offset ("Gauge offset"): (offsets, stds, optimal_pad) with offsets = np.arange(hop), stds float64 (hop,)
    numpy -- for pad i the standard deviation over the frames of the band mean of the STFT of `channel` with i zeros in front --
    and optimal_pad = int(np.argmax(stds)), the first maximum.  numpy or device input, (n,) or (n, ch); never modified."""
    dev = _dev.device_index(device if device is not None else (signal.device if torch.is_tensor(signal) else None))
    s2d = _as_2d(signal)
    if not 0 <= channel < s2d.shape[1]:
        raise IndexError(f"channel {channel} of a {s2d.shape[1]}-channel signal")
    col = s2d[:, channel]                                            # only this channel goes to the device
    stds = _dev.to_host(sniff_offset_dev(_dev.to_dev(col, torch.float32, dev), sr, fft_size, hop, 0, band, dev))
    return np.arange(int(hop)), stds, int(np.argmax(stds))


def _check_offset(offset, hop):
    offset = int(offset)
    if not 0 <= offset < hop:
        raise ValueError(f"offset {offset} outside 0 <= offset < hop ({hop})")
    return offset


def fused_supported(fft_size, hop):
    """par_gate_stft_f32 takes power-of-two transforms of 16..8192 points with 1 <= hop <= n_fft."""
    return 16 <= fft_size <= 8192 and (fft_size & (fft_size - 1)) == 0 and 1 <= hop <= fft_size


def _check_channels(channels, ch):
    chans = [int(c) for c in channels]
    if len(set(chans)) != len(chans):
        raise ValueError(f"channels {chans} repeat a channel")
    for c in chans:
        if c >= len(chans) or c >= ch or c < 0:
            raise IndexError(f"index {c} is out of bounds for axis 1 with size {min(len(chans), ch)}")
    return chans


def renoise_dev(sig_t, final, gain=GAIN, fft_size=FFT_SIZE, hop=FFT_SIZE // OVERLAP, channels=None, dev=None, fused=None, out=None,
                offset=0):
    """Device form of renoise: sig_t float32 (n, ch) device tensor -> float32 (n, len(channels)) device tensor.  fused: None
    picks by size (par_gate_stft_f32 up to 8192 points), False forces the composed path (K_stft -> par_gate_spectrum_f32 ->
    K_istft per channel; the tests' reference for the fused kernel).  offset: zeros in front of every channel before the
    STFT, dropped from the result (0 <= offset < hop; 0 is the path without the argument)."""
    offset = _check_offset(offset, hop)
    dev = _dev.device_index(dev if dev is not None else sig_t.device)
    if offset:
        n0, ch0 = sig_t.shape
        padded = torch.zeros((n0 + offset, ch0), dtype=torch.float32, device=f"cuda:{dev}")
        padded[offset:] = sig_t
        res = renoise_dev(padded, final, gain, fft_size, hop, channels, dev, fused)[offset:]
        if out is None:
            return res
        out.copy_(res)
        return out
    L = _lib.lib()
    n, ch = sig_t.shape
    chans = _check_channels(range(ch) if channels is None else channels, ch)
    k = len(chans)
    if k == 0:
        raise ValueError("no channel selected")
    bins = fft_size // 2 + 1
    thr = np.asarray(final, dtype=np.float64)
    if thr.shape != (bins,):
        raise ValueError(f"final profile has {thr.shape} bins, the FFT size {fft_size} has {bins}")
    cut_t = _dev.to_dev(gate_cutoffs(thr), torch.float32, dev)
    low = float(low_factor(gain))
    window_t = fourier.window_dev(WINDOW, fft_size, dev)
    if out is None:
        out = _dev.empty((n, k), torch.float32, dev)
    use_fused = fused_supported(fft_size, hop) if fused is None else fused
    stream = _dev.stream_ptr(dev)
    if use_fused:
        # channels are a permutation of 0..k-1 (checked above): channel c -> column c, all in one launch
        _lib.check(L.par_gate_stft_f32(dev, _dev.ptr(sig_t), n, ch, k, fft_size, hop, _dev.ptr(window_t), _dev.ptr(cut_t), low,
                                       _dev.ptr(out), out.stride(0), stream))
        return out
    half = fft_size // 2
    for c in chans:
        xpad = torch.zeros(n + half, dtype=torch.float32, device=f"cuda:{dev}")        # fourier.fix_length(sig, n + n_fft // 2)
        xpad[:n] = sig_t[:, c]
        spec = fourier.stft_dev(xpad, fft_size, hop, window_t, 1, 0, dev=dev)         # (bins, frames) view of [frames][bins]
        fm = spec.T
        _lib.check(L.par_gate_spectrum_f32(dev, _dev.ptr(fm), fm.shape[0], bins, 0, _dev.ptr(cut_t), low, stream))
        out[:, c] = fourier.istft_dev(spec, hop, window_t, length=n, dev=dev)
    return out


def renoise_offset(signal, sr, final, offset, gain=GAIN, fft_size=FFT_SIZE, hop=FFT_SIZE // OVERLAP, channels=None, device=None):
    """renoise with the frames starting `offset` samples earlier (sniff_offset's optimal_pad; experiments/renoiser.py:60-65):
    `offset` zeros go in front of every selected channel before the STFT and are dropped from the result.  0 <= offset < hop,
    else ValueError before any device work; offset 0 is renoise's own path.  Input and result as renoise."""
    offset = _check_offset(offset, hop)
    dev = _dev.device_index(device if device is not None else (signal.device if torch.is_tensor(signal) else None))
    was_tensor = torch.is_tensor(signal)
    sig2d = _as_2d(signal)
    sig_t = _dev.to_dev(sig2d, torch.float32, dev).contiguous()
    out = renoise_dev(sig_t, final, gain, fft_size, hop, channels, dev, offset=offset)
    res = out if signal.ndim == 2 else out[:, 0]
    return res if was_tensor else _dev.to_host(res)


def renoise(signal, sr, final, gain=GAIN, fft_size=FFT_SIZE, hop=FFT_SIZE // OVERLAP, channels=None, device=None):
    """run_resample of the GUI on an (n, ch) (or (n,)) float32 signal: returns float32 (n, len(channels)) -- numpy for numpy
    input, a device tensor for a tensor; a 1-D input gives a 1-D result.  channels: the selected channel numbers (default
    all).  `final` is the float64 threshold profile (final_profile), `gain` the dB every bin at or under it gets."""
    return renoise_offset(signal, sr, final, 0, gain, fft_size, hop, channels, device)


def output_path(path, fft_size):
    """The file run_resample writes: io_ops.write_file(path, ..., suffix=f" fft={fft_size}")"""
    return f"{os.path.splitext(path)[0]} fft={fft_size}.wav"


def renoise_file(path, noise_path=None, selection=None, fft_size=FFT_SIZE, overlap=OVERLAP, gain=GAIN, overhead=OVERHEAD,
                 curve=None, channels=None, device=None, signal_data=None, resample_noise=False, offset=0):
    """The GUI's flow on a file: read `path` (signal_data=(signal, sr, channels) skips the read); the noise profile comes from
    the noise file `noise_path` (same rate, or any rate with resample_noise=True), from the time range selection=(t0, t1) of channel 0, or is the -100 dB default;
    apply and write "<stem> fft=<N>.wav" (float32 WAV).  Returns the written path, or None when no channel is selected (the
    reference then writes nothing).  offset: 0 <= offset < hop as in renoise_offset, or "auto" for sniff_offset's optimal_pad of
    channel 0."""
    if noise_path is not None and selection is not None:
        raise ValueError("give a noise file or a selection, not both")
    hop = fft_size // overlap
    if offset != "auto":
        offset = _check_offset(offset, hop)
    dev = _dev.device_index(device)
    signal, sr, num_channels = io_ops.read_file(path) if signal_data is None else signal_data
    chans = list(range(_as_2d(signal).shape[1])) if channels is None else list(channels)
    if not chans:
        return None
    sig_t = _dev.to_dev(_as_2d(signal), torch.float32, dev).contiguous()
    if noise_path is not None:
        noise, noise_sr, _ = io_ops.read_file(noise_path)
        prof = noise_profile(noise, noise_sr, sr, fft_size, hop, dev, resample_noise=resample_noise)
    elif selection is not None:
        prof = noise_profile_from_selection(sig_t, sr, selection[0], selection[1], fft_size, hop, 0, dev)
    else:
        prof = default_profile(sr, fft_size)
    final = final_profile(prof, sr, fft_size, gain, overhead, curve)
    if offset == "auto":
        offset = int(np.argmax(_dev.to_host(sniff_offset_dev(sig_t, sr, fft_size, hop, 0, dev=dev))))
        logging.info("%s: gauged offset %d", path, offset)
    out = _dev.to_host(renoise_dev(sig_t, final, gain, fft_size, hop, chans, dev, offset=offset))
    io_ops.write_file(path, out, sr, len(chans), suffix=f" fft={fft_size}")
    return output_path(path, fft_size)
