"""Mirror of reference util/spectrum_flat.py:1-43 -- time-averaged dB spectra of a file (the analysis under the Spectral Expander,
humspeed and difeq).  Same names, signatures, defaults and return types; the STFT runs in K_stft and the temporal mean of the dB
spectrogram in K_expand (par_mean_db_frames_f32) over frame chunks, so no full spectrogram is held however long the file.

Device-level helpers: `mag_chunks_dev` (frame-chunked magnitude spectrogram), `mean_spectrum_db_dev` (float64 temporal mean of the
dB spectrum of one channel, a device tensor), `mean_spectra_db_dev` (the same for several channels of an interleaved signal,
straight from the samples in one launch of par_stft_mean_db_f32 where the size allows: difeq's path) and `band_db_curve_dev` (the
per-frame mean dB of a band of bins)."""
import logging

import numpy as np
import torch

from . import _dev, _lib, fourier, io_ops

channel_map = {"L": (0,), "R": (1,), "L+R": (0, 1), "Mean": (0, 1)}

# spectrogram rows (plus the four-step transform's scratch) held at once by the frame-chunked paths
CHUNK_BYTES = 512 << 20


def _frames(n, n_fft, hop):
    return int(_lib.lib().par_stft_frames(n, n_fft, hop))


def mag_chunks_dev(x_t, n_fft, hop, window_t, zeropad=1, x_stride=1, n=None, dev=None, chunk_bytes=CHUNK_BYTES):
    """Yield (f0, f1, fm): the magnitude rows |X| / sqrt(n_fft) + 1e-7 of frames [f0, f1) of x_t (float32 device tensor, element
    stride x_stride, logical length n) as a frame-major float32 view fm[f1 - f0, bins] (row stride >= bins), equal to the rows
    fourier.get_mag computes on the whole signal.  A chunk is the STFT of a window of the signal that starts a few frames early
    (those frames, whose reflect padding differs, are dropped) and ends where the chunk's last frame ends, or at the signal's end."""
    dev = _dev.device_index(dev if dev is not None else x_t.device)
    if n is None:
        n = x_t.numel() // x_stride
    n_frames = _frames(n, n_fft, hop)
    M = n_fft * zeropad
    bins = M // 2 + 1
    per_frame = 4 * bins + (8 * M if M > 16384 else 0)
    chunk = max(1, chunk_bytes // per_frame)
    half = n_fft // 2
    lead_max = -(-half // hop)                      # frames whose window starts before the signal
    for f0 in range(0, n_frames, chunk):
        f1 = min(n_frames, f0 + chunk)
        s = max(0, f0 - lead_max)
        lead = f0 - s
        n_sub = n - s * hop
        if f1 < n_frames:
            n_sub = min(n_sub, (f1 - 1 - s) * hop + n_fft - half)
        sub = x_t[s * hop * x_stride:]
        mag = fourier.stft_dev(sub, n_fft, hop, window_t, zeropad, 1, x_stride=x_stride, n=n_sub, dev=dev)
        yield f0, f1, mag.T[lead:lead + f1 - f0]


def mean_spectrum_db_dev(x_t, fft_size, hop, window="hann", zeropad=1, x_stride=1, n=None, dev=None, chunk_bytes=CHUNK_BYTES):
    """np.mean(to_dB(get_mag(x, fft_size, hop, window)), axis=1) of one channel as a float64 device tensor (bins,): the dB of every
    frame is summed per bin in float64 (fixed order) over frame chunks and divided by the frame count."""
    dev = _dev.device_index(dev if dev is not None else x_t.device)
    L = _lib.lib()
    window_t = fourier.window_dev(window, fft_size, dev)
    bins = fft_size * zeropad // 2 + 1
    acc = torch.zeros(bins, dtype=torch.float64, device=f"cuda:{dev}")
    total = 0
    for f0, f1, fm in mag_chunks_dev(x_t, fft_size, hop, window_t, zeropad, x_stride, n, dev, chunk_bytes):
        _lib.check(L.par_mean_db_frames_f32(dev, _dev.ptr(fm), f1 - f0, bins, fm.stride(0), _dev.ptr(acc), _dev.stream_ptr(dev)))
        total = f1
    return acc / total


def fused_mean_supported(fft_size, zeropad=1):
    """Sizes par_stft_mean_db_f32 takes: n_fft * zeropad a power of two in [16, 16384]"""
    m = int(fft_size) * int(zeropad)
    return fft_size % 2 == 0 and 16 <= m <= 16384 and m & (m - 1) == 0


# mean_spectra_db_dev's default path (fused=None): True = straight from the samples (par_stft_mean_db_f32) wherever the size
# allows.  Measured on stereo (tools/bench_difeq.py): 2.9x to 3.5x ahead of the chunked path at 16384 / 8192, 15x at 4096 / 256.
FUSED_MEAN = True


def mean_spectra_db_dev(sig_t, fft_size, hop, channels, window="hann", zeropad=1, fused=None, dev=None):
    """mean_spectrum_db_dev of the channels `channels` of the interleaved device signal sig_t (n, ch) float32 -> float64 device
    tensor (len(channels), bins).  fused (default FUSED_MEAN): all channels in one launch straight from the samples
    (par_stft_mean_db_f32, up to 16384 points, at most 8 channels), no spectrogram stored; otherwise, and for the sizes that
    kernel does not take, the chunked mean_spectrum_db_dev channel by channel.  The two differ in the order of the float64 sums."""
    dev = _dev.device_index(dev if dev is not None else sig_t.device)
    if sig_t.ndim != 2 or sig_t.dtype != torch.float32 or not sig_t.is_contiguous():
        raise ValueError("signal must be a contiguous (n, channels) float32 tensor")
    n, ch = sig_t.shape
    channels = tuple(int(c) for c in channels)
    if not channels or not all(0 <= c < ch for c in channels):
        raise ValueError(f"channels {channels} of a {ch}-channel signal")
    bins = fft_size * zeropad // 2 + 1
    x_t = sig_t.reshape(-1)
    if (FUSED_MEAN if fused is None else fused) and fused_mean_supported(fft_size, zeropad) and ch <= 8:
        L = _lib.lib()
        window_t = fourier.window_dev(window, fft_size, dev)
        # one launch over the file's channels when they are asked for in file order from the first on, else one per channel
        whole = channels == tuple(range(len(channels)))
        groups = [(0, len(channels))] if whole else [(c, 1) for c in channels]
        out = _dev.empty((len(channels), bins), torch.float64, dev)
        nbytes = int(L.par_stft_mean_db_scratch_bytes(n, fft_size, hop, zeropad, groups[0][1]))
        scratch = _dev.empty(nbytes // 8, torch.float64, dev)
        for i, (c0, n_ch) in enumerate(groups):
            _lib.check(L.par_stft_mean_db_f32(dev, _dev.ptr(x_t[c0:]), n, ch, n_ch, fft_size, hop, zeropad, _dev.ptr(window_t),
                                              _dev.ptr(out[i:]), _dev.ptr(scratch), nbytes, _dev.stream_ptr(dev)))
        return out
    return torch.stack([mean_spectrum_db_dev(x_t[c:], fft_size, hop, window, zeropad, x_stride=ch, n=n, dev=dev) for c in channels])


def band_db_curve_dev(x_t, fft_size, hop, bin_l, bin_u, window="hann", zeropad=1, x_stride=1, n=None, fused=True, dev=None, out=None,
                      chunk_bytes=CHUNK_BYTES):
    """Per frame, the mean over bins [bin_l, bin_u) of 20 log10(magnitude) -- np.mean(to_dB(get_mag(x))[bin_l:bin_u], axis=0) in
    float64 -- as a float64 device tensor (frames,).  fused: straight out of the STFT kernel (par_stft_band_db_f32, up to 16384
    points); otherwise (and above 16384 points) the magnitude rows of frame chunks and par_band_mean_db_f32."""
    dev = _dev.device_index(dev if dev is not None else x_t.device)
    L = _lib.lib()
    if n is None:
        n = x_t.numel() // x_stride
    frames = _frames(n, fft_size, hop)
    if out is None:
        out = _dev.empty(frames, torch.float64, dev)
    window_t = fourier.window_dev(window, fft_size, dev)
    if fused and fft_size * zeropad <= 16384:
        _lib.check(L.par_stft_band_db_f32(dev, _dev.ptr(x_t), n, x_stride, fft_size, hop, zeropad, _dev.ptr(window_t), bin_l, bin_u,
                                          _dev.ptr(out), _dev.stream_ptr(dev)))
        return out
    bins = fft_size * zeropad // 2 + 1
    for f0, f1, fm in mag_chunks_dev(x_t, fft_size, hop, window_t, zeropad, x_stride, n, dev, chunk_bytes):
        _lib.check(L.par_band_mean_db_f32(dev, _dev.ptr(fm), f1 - f0, bins, fm.stride(0), bin_l, bin_u, 0, f1 - f0, _dev.ptr(out[f0:]),
                                          _dev.stream_ptr(dev)))
    return out


def spectra_from_audio(filename, fft_size=4096, hop=256, channel_mode="L", temporal_mean=True):
    signal, sr, num_channels = io_ops.read_file(filename)
    dev = _dev.device_index(None)
    sig2d = signal if signal.ndim == 2 else signal[:, None]
    sig_t = _dev.to_dev(sig2d, torch.float32, dev)
    x_t = sig_t.reshape(-1)
    n, ch = sig2d.shape
    spectra = []
    for channel in channel_map[channel_mode]:
        logging.debug(f"channel {channel}")
        if channel == num_channels:
            logging.warning("not enough channels for L/R comparison  - fallback to mono")
            break
        if temporal_mean:
            # float64, the dtype of the reference's CPU backends (the CUDA one gives float32)
            spec = _dev.to_host(mean_spectrum_db_dev(x_t[channel:], fft_size, hop, "hann", x_stride=ch, n=n, dev=dev))
        else:
            # the reference's own host arithmetic on the downloaded spectrogram (util/units.py:24-25 on float32)
            mag = fourier.stft(sig_t[:, channel], fft_size, hop, "hann", _mode=1)
            spec = 20 * np.log10(_dev.to_host(mag))
        spectra.append(spec)
    # take mean across channels
    if channel_mode == "Mean":
        spectra = [np.mean(spectra, axis=0), ]
    return spectra, sr


def spectrum_from_audio(filename, fft_size=4096, hop=256, channel_mode="L", temporal_mean=True):
    spectra, sr = spectra_from_audio(filename, fft_size, hop, channel_mode, temporal_mean)
    if len(spectra) > 1:
        return np.mean(spectra, axis=0), sr
    else:
        return spectra[0], sr


def spectrum_from_audio_stereo(filename, fft_size=4096, hop=256, channel_mode="L", temporal_mean=True):
    spectra, sr = spectra_from_audio(filename, fft_size, hop, channel_mode, temporal_mean)
    if len(spectra) < 2:
        spectra.append(spectra[0])
    return spectra, sr
