"""The stereo balance tool of the reference (pypan_gui.py) on the GPU, headless.

    samples = pan_samples(signal, sr, [((12.0, 300.0), (14.5, 5000.0))], 4096, 8)    # the Shift-drag of pypan_gui.py:78-104
    curve = pan_line(samples, len(signal) / sr, sr, 4096 // 8)                        # markers.PanLine.update
    right = apply_pan(signal, sr, curve)                                              # Canvas.run_resample without the file
    process("tape.wav", boxes=[(12.0, 300.0, 14.5, 5000.0)])                          # ... and with it: writes tape_out.wav

A box measures fac = np.nanmean(L[bL:bU, f0:f1] / R[bL:bU, f0:f1]) on the float32 magnitude spectrograms of two channels; the
markers' (t, fac) pairs are joined by np.interp into the pan line, and the right channel is multiplied by that line.  Here all
boxes of a file are measured in ONE launch straight from the interleaved samples (par_stft_pan_ratio_f32: no spectrogram is
stored, only frames inside a box are transformed); FFT sizes that kernel does not take go through two magnitude spectrograms and
par_pan_ratio_f32.  The curve is applied by par_pan_apply_f32, numpy's np.interp bit for bit.  There is no CPU path."""
import json
import logging
import os

import numpy as np
import torch

from . import _dev, _lib, fourier, io_ops

# True: measure straight from the samples (par_stft_pan_ratio_f32) wherever the size allows; False: always through two stored
# magnitude spectrograms.  Measured (tools/bench_pypan.py, NOTES.md "Stereo balance (pypan)"): 10 min of stereo, 4096 points, 1 / 8 /
# 64 boxes of 3 s: 0.05 / 0.08 / 0.31 ms fused against 0.8 ms composed, the same result bit for bit -- fused is the default.
FUSED = True
WINDOW = "blackmanharris"                   # util/spectrum.py:385
EXT = ".pan"                                # pypan_gui.py:9
EMPTY_LINE = ((0.0, 0.0), (999.0, 0.0))     # BaseLine.empty (util/markers.py:571-573)


class PanSample:
    """What markers.PanSample (util/markers.py:325-363) keeps of a measurement: the two clicks, the factor, the marker's time."""

    def __init__(self, a, b, pan):
        self.a = (a[0], a[1])
        self.b = (b[0], b[1])
        self.pan = pan
        self.t = (a[0] + b[0]) / 2

    def to_cfg(self):
        return self.a[0], self.a[1], self.b[0], self.b[1], self.pan

    @classmethod
    def from_cfg(cls, a0, a1, b0, b1, pan):
        return cls((a0, a1), (b0, b1), pan)

    def __repr__(self):
        return f"PanSample(a={self.a}, b={self.b}, pan={self.pan!r})"


def _as_sample(m):
    return m if isinstance(m, PanSample) else PanSample.from_cfg(*m)


def _as_box(box):
    """((t, f), (t, f)) or (t0, f0, t1, f1) -> (a, b)"""
    if len(box) == 4:
        return (box[0], box[1]), (box[2], box[3])
    a, b = box
    return (a[0], a[1]), (b[0], b[1])


def box_to_cells(a, b, sr, fft_size, hop, num_bins, n_frames):
    """The integers pypan_gui.py:81-98 derives from the clicks a = (t, f), b = (t, f): (bin_l, bin_u, frame_0, frame_1), half-open.
    Quirks kept: a time of exactly 0 is falsy and leaves its end of the range alone; the frequencies meet Python's round (ties to
    even) and fft_size WITHOUT the zero-padding factor; bins are clamped to [1, num_bins - 3]."""
    t0, t1 = sorted((a[0], b[0]))
    freqs = sorted((a[1], b[1]))
    f_l = max(freqs[0], 1)
    f_u = min(freqs[1], sr // 2 - 1)
    first, last = 0, n_frames
    if t0:
        first = max(first, int(t0 * sr / hop))
    if t1:
        last = min(last, int(t1 * sr / hop))

    def freq2bin(f):
        return max(1, min(num_bins - 3, int(round(f * fft_size / sr))))
    return freq2bin(f_l), freq2bin(f_u), first, last


def _clamped(cells, num_bins, n_frames):
    """numpy's slice semantics for the reference's L[bL:bU, first:last]: ends beyond the array stop at it (a first frame behind the
    file, a negative time), which leaves the selected cells as they are and keeps every box inside the spectrogram."""
    out = np.empty((len(cells), 4), dtype=np.int32)
    for i, (bl, bu, f0, f1) in enumerate(cells):
        b0, b1, _ = slice(bl, bu).indices(num_bins)
        g0, g1, _ = slice(f0, f1).indices(n_frames)
        out[i] = (b0, b1, g0, g1)
    return out


def _boxes(cells, num_bins, n_frames, dev):
    host = _clamped(cells, num_bins, n_frames)
    return host, _dev.to_dev(host, torch.int32, dev)


def pan_ratio_dev(L_t, R_t, cells, dev=None, with_count=False):
    """fac of every box of `cells` = [(bin_l, bin_u, frame_0, frame_1), ...] on two device magnitude spectrograms of logical shape
    (bins, frames) over frame-major memory -- what fourier.stft_dev(mode=1) returns, pitched rows included.  -> float64 device
    tensor (n_box,), with with_count also the int64 cell counts."""
    dev = _dev.device_index(dev if dev is not None else L_t.device)
    L = _lib.lib()
    if L_t.shape != R_t.shape or L_t.ndim != 2:
        raise ValueError("L and R must be two (bins, frames) spectrograms of one shape")
    fm = []
    for t in (L_t, R_t):
        t = t if t.dtype == torch.float32 else t.to(torch.float32)
        fm.append(t.T if t.T.stride(1) == 1 and t.T.stride(0) >= t.shape[0] else t.T.contiguous())
    if fm[0].stride(0) != fm[1].stride(0):
        fm = [t.contiguous() for t in fm]
    bins, frames = L_t.shape
    n_box = len(cells)
    fac = _dev.empty(n_box, torch.float64, dev)
    count = _dev.empty(n_box, torch.int64, dev)
    if n_box:
        host, boxes = _boxes(cells, bins, frames, dev)
        nbytes = int(L.par_pan_ratio_scratch_bytes(host.ctypes.data, n_box))
        scratch = _dev.empty(nbytes // 8, torch.int64, dev)
        _lib.check(L.par_pan_ratio_f32(dev, _dev.ptr(fm[0]), _dev.ptr(fm[1]), frames, bins, fm[0].stride(0), _dev.ptr(boxes),
                                       host.ctypes.data, n_box, _dev.ptr(fac), _dev.ptr(count), _dev.ptr(scratch), nbytes,
                                       _dev.stream_ptr(dev)))
    return (fac, count) if with_count else fac


def pan_ratio(L, R, cells, device=None):
    """np.nanmean(L[bL:bU, f0:f1] / R[bL:bU, f0:f1]) for every box, L and R numpy magnitude spectrograms in the reference's
    (bins, frames) orientation -> float64 (n_box,)."""
    dev = _dev.device_index(device)
    L_t = _dev.to_dev(np.asarray(L).T, torch.float32, dev).T
    R_t = _dev.to_dev(np.asarray(R).T, torch.float32, dev).T
    return _dev.to_host(pan_ratio_dev(L_t, R_t, cells, dev))


def fused_supported(fft_size, zeropad=1):
    """Sizes par_stft_pan_ratio_f32 takes: n_fft * zeropad a power of two in [16, 16384]"""
    m = int(fft_size) * int(zeropad)
    return fft_size % 2 == 0 and 16 <= m <= 16384 and m & (m - 1) == 0


def pan_samples_dev(sig_t, sr, boxes, fft_size, fft_overlap, zeropad=1, channels=(0, 1), window_name=WINDOW, dev=None, fused=None):
    """pan_samples on a device signal (n, ch) float32 (interleaved) -> (float64 device tensor (n_box,), cells)"""
    dev = _dev.device_index(dev if dev is not None else sig_t.device)
    L = _lib.lib()
    if sig_t.ndim != 2 or sig_t.dtype != torch.float32 or not sig_t.is_contiguous():
        raise ValueError("signal must be a contiguous (n, channels) float32 tensor")
    n, ch = sig_t.shape
    c_l, c_r = channels
    if not (0 <= c_l < ch and 0 <= c_r < ch):
        raise ValueError(f"channels {channels} of a {ch}-channel signal")
    hop = fft_size // fft_overlap
    num_bins = fft_size * zeropad // 2 + 1
    n_frames = int(L.par_stft_frames(n, fft_size, hop))
    cells = [box_to_cells(*_as_box(b), sr, fft_size, hop, num_bins, n_frames) for b in boxes]
    window = fourier.window_dev(window_name, fft_size, dev)
    x_l, x_r = sig_t[:, c_l], sig_t[:, c_r]
    if (FUSED if fused is None else fused) and fused_supported(fft_size, zeropad):
        n_box = len(cells)
        fac = _dev.empty(n_box, torch.float64, dev)
        if n_box:
            count = _dev.empty(n_box, torch.int64, dev)
            host, boxes_t = _boxes(cells, num_bins, n_frames, dev)
            nbytes = int(L.par_stft_pan_scratch_bytes(host.ctypes.data, n_box))
            scratch = _dev.empty(nbytes // 8, torch.int64, dev)
            _lib.check(L.par_stft_pan_ratio_f32(dev, _dev.ptr(x_l), _dev.ptr(x_r), ch, n, fft_size, hop, zeropad, _dev.ptr(window),
                                                _dev.ptr(boxes_t), host.ctypes.data, n_box, _dev.ptr(fac), _dev.ptr(count),
                                                _dev.ptr(scratch), nbytes, _dev.stream_ptr(dev)))
        return fac, cells
    mags = [fourier.stft_dev(x, fft_size, hop, window, zeropad, mode=1, x_stride=ch, n=n, dev=dev) for x in (x_l, x_r)]
    return pan_ratio_dev(mags[0], mags[1], cells, dev), cells


def pan_samples(signal, sr, boxes, fft_size, fft_overlap, zeropad=1, channels=(0, 1), window_name=WINDOW, device=None):
    """The Shift-drag of pypan_gui.py:78-104 for every box of `boxes` = [((t, f), (t, f)) or (t0, f0, t1, f1), ...] on the
    (n, channels) float32 signal: -> [PanSample] in the order given.  hop = fft_size // fft_overlap (util/widgets.py:398)."""
    dev = _dev.device_index(device)
    sig_t = signal if isinstance(signal, torch.Tensor) else _dev.to_dev(np.asarray(signal), torch.float32, dev)
    fac, _ = pan_samples_dev(sig_t, sr, boxes, fft_size, fft_overlap, zeropad, channels, window_name, dev)
    fac = _dev.to_host(fac)
    return [PanSample(*_as_box(b), float(v)) for b, v in zip(boxes, fac)]


def pan_line(markers, duration, sr, hop):
    """markers.PanLine.update (util/markers.py:711-727): the markers (PanSample, or their to_cfg() tuples) sorted by time and
    joined by np.interp at BaseLine.get_times() = np.linspace(0, duration, int(duration * sr / hop)) -> (num, 2) float64 rows
    (time, pan).  Without markers: BaseLine.empty, the float32 rows (0, 0), (999, 0), as the reference leaves it."""
    markers = [_as_sample(m) for m in markers]
    if not markers:
        return np.array(EMPTY_LINE, dtype=np.float32)
    markers.sort(key=lambda m: m.t)
    times = np.linspace(0, duration, num=int(duration * (sr / hop)))
    pan = np.interp(times, [m.t for m in markers], [m.pan for m in markers])
    return np.stack((times, pan), axis=-1)


def apply_pan_dev(sig_t, sr, pan_curve, channel=1, dev=None, out=None):
    """float32(float64(signal[:, channel]) * np.interp(arange(n), pan_curve[:, 0] * sr, pan_curve[:, 1])) on a device signal
    (n, ch) or (n,) float32 -> float32 device tensor (n,) (`out`: a float32 view of n elements to fill, any stride)."""
    dev = _dev.device_index(dev if dev is not None else sig_t.device)
    L = _lib.lib()
    if sig_t.dtype != torch.float32:
        raise ValueError("signal must be float32")
    x = sig_t[:, channel] if sig_t.ndim == 2 else sig_t
    n = x.shape[0]
    curve = np.asarray(pan_curve)
    xp = _dev.to_dev(curve[:, 0] * sr, torch.float64, dev)            # the product in the curve's own precision, as numpy forms it
    fp = _dev.to_dev(curve[:, 1], torch.float64, dev)
    if out is None:
        out = _dev.empty(n, torch.float32, dev)
    if out.shape != (n,) or out.dtype != torch.float32:
        raise ValueError("out must be a float32 tensor of n elements")
    _lib.check(L.par_pan_apply_f32(dev, _dev.ptr(x), x.stride(0) if n > 1 else 1, n, _dev.ptr(xp), _dev.ptr(fp), xp.numel(),
                                   _dev.ptr(out), out.stride(0) if n > 1 else 1, _dev.stream_ptr(dev)))
    return out


def apply_pan(signal, sr, pan_curve, channel=1, device=None):
    """Canvas.run_resample's product (pypan_gui.py:57-58) as the FLOAT file stores it: float32 (n,)"""
    dev = _dev.device_index(device)
    signal = np.asarray(signal)
    x = signal[:, channel] if signal.ndim == 2 else signal
    return _dev.to_host(apply_pan_dev(_dev.to_dev(x, torch.float32, dev), sr, pan_curve, dev=dev))


def save_project(path, cfg):
    """Write a .pan project with the keys ParamWidget.save writes for this tool (util/widgets.py:1224-1233, :326): fft_size,
    fft_overlap, fft_zeropad and "markers" (PanSample.to_cfg() rows), in the reference's JSON layout (util/config.py:17-21).
    Other keys of `cfg` are kept."""
    out = dict(cfg)
    out["markers"] = [list(_as_sample(m).to_cfg()) for m in cfg.get("markers", ())]
    for key in ("fft_size", "fft_overlap", "fft_zeropad"):
        out[key] = int(cfg[key])
    with open(path, "w") as f:
        json.dump(out, f, indent="\t", sort_keys=True)


def process(path=None, project=None, boxes=None, out_suffix="_out", keep_left=False, fft_size=4096, fft_overlap=8, zeropad=1,
            device=None, apply=True):
    """Run the tool on a file: the markers of a .pan `project` (a path or the dict; its fft_size / fft_overlap give the line's
    hop, its "source" the file when `path` is None), or markers measured in `boxes` with the given FFT settings, or both
    (measured ones are appended); then PanLine.update and run_resample, which writes ONLY the corrected right channel, mono,
    as <stem><out_suffix>.wav.  keep_left=True is an extension of this port: a stereo file with the untouched left channel
    beside the corrected right one.  apply=False only measures.  Without any marker nothing is written, as in the reference
    (:54).  -> (output path or None, [PanSample])"""
    dev = _dev.device_index(device)                   # no GPU: stop before touching a file
    markers = []
    if project is not None:
        cfg = project if isinstance(project, dict) else json.load(open(project))
        fft_size, fft_overlap = int(cfg.get("fft_size", fft_size)), int(cfg.get("fft_overlap", fft_overlap))
        zeropad = int(cfg.get("fft_zeropad", zeropad))
        markers = [PanSample.from_cfg(*m) for m in cfg.get("markers", ())]
        path = path or cfg.get("source")
    if not path:
        raise ValueError("no audio file: give `path` or a project with a \"source\"")
    signal, sr, ch = io_ops.read_file(path)
    if ch < 2:
        raise ValueError(f"{path}: the balance tool needs two channels, the file has {ch}")
    sig_t = _dev.to_dev(signal, torch.float32, dev)
    if boxes:
        fac, _ = pan_samples_dev(sig_t, sr, boxes, fft_size, fft_overlap, zeropad, dev=dev)
        markers += [PanSample(*_as_box(b), float(v)) for b, v in zip(boxes, _dev.to_host(fac))]
    if not apply:
        return None, markers
    if not markers:
        logging.warning("%s: no markers, nothing written", path)
        return None, markers
    curve = pan_line(markers, len(signal) / sr, sr, fft_size // fft_overlap)
    if keep_left:
        out_t = sig_t[:, :2].clone()
        apply_pan_dev(sig_t, sr, curve, 1, dev, out=out_t[:, 1])
    else:
        out_t = apply_pan_dev(sig_t, sr, curve, 1, dev)
    io_ops.write_file(path, _dev.to_host(out_t), sr, 2 if keep_left else 1, suffix=out_suffix)
    return f"{os.path.splitext(path)[0]}{out_suffix}.wav", markers
