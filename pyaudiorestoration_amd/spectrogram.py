"""The spectrogram picture of the reference (util/spectrum.py, util/vispy_ext.MelTransform) on the GPU, headless.

    rgba, geo = render(signal, sr, width=2048, height=1024)           # (height, width, 4) uint8 and the ImageGeometry
    t, f = geo.to_time_freq(x, y)                                     # what pixel (x, y) shows, in (s, Hz)
    render_file("tape.flac")                                          # tape_spec.png + tape_spec.json

Every tool of the port takes (seconds, Hz) pairs that the reference's user reads off this picture.  The arithmetic of the display
is the whole-file STFT, its dB values and their reduction to a screen's pixels; here the reduction is PEAK HOLD (a pilot tone one
frame wide survives it, and a maximum has no summation order), fused into the transform: par_stft_peak_image_f32 stores no
spectrogram.  FUSED = False, and every transform above 16384 points, takes stored magnitude chunks and par_peak_image_f32; the two
routes give the same bits.  Colours are a separate pass (par_image_colorize_u8), so new limits or another colour map cost nothing
but that pass.  Axes, text, markers and interaction stay with the GUI.  There is no CPU path for the picture."""
import json
import os
import struct
import zlib

import numpy as np
import torch

from . import _dev, _lib, fourier, io_ops

# True: the peak image comes straight from the samples (par_stft_peak_image_f32) wherever the size allows; False: always from
# stored magnitude chunks (par_stft_f32 mode 1 + par_peak_image_f32).  The rule (NOTES.md "Spectrogram image"): the fused route is
# the default only over the sizes where tools/bench_spectrogram.py measured it no slower than the composed one.  That bench has not
# run on the device yet, so nothing is measured and the default is the composed route; the two give the same bits either way.
FUSED = False
SCALES = ("mel", "linear", "log")
VMIN, VMAX = -120.0, 0.0                   # util/spectrum.py:233-234


def fused_supported(fft_size, zeropad=1):
    """The sizes par_stft_peak_image_f32 takes: fft_size * zeropad a power of two in [16, 16384], fft_size even"""
    M = int(fft_size) * int(zeropad)
    return fft_size >= 2 and zeropad >= 1 and fft_size % 2 == 0 and 16 <= M <= 16384 and M & (M - 1) == 0


def stft_frames(n, fft_size, hop):
    """par_stft_frames: frames of the centred, reflect-padded STFT of n samples"""
    if n < 1 or fft_size < 1 or hop < 1:
        return 0
    return (n + 2 * (fft_size // 2) - fft_size) // hop + 1


def _scale_fwd(scale, f):
    f = np.asarray(f, dtype=np.float64)
    if scale == "mel":
        return np.log(f / 700.0 + 1.0) * 1127.0                 # util/units.py:42-47
    if scale == "log":
        return np.log2(f)
    return f


def _scale_inv(scale, y):
    y = np.asarray(y, dtype=np.float64)
    if scale == "mel":
        return (np.exp(y / 1127.0) - 1.0) * 700.0
    if scale == "log":
        return np.exp2(y)
    return y


def _snap(e):
    """A column edge within 1e-9 frames (relative above one frame) of a whole frame IS that frame: the float64 expression of an
    edge carries a few 1e-16 of rounding, which at a one-to-one zoom would put every other edge just under its frame and tear the
    columns apart; 1e-9 frames is some 1e-12 s, far below anything a marker can mean."""
    e = np.asarray(e, dtype=np.float64)
    k = np.rint(e)
    return np.where(np.abs(e - k) <= 1e-9 * np.maximum(1.0, np.abs(e)), k, e)


class ImageGeometry:
    """Which frames a column and which bins a row of the picture hold; built by geometry().

    col_lo, col_hi: int64[width], half-open frame ranges; row_lo, row_hi: int32[height], half-open bin ranges, row 0 on top.
    Frame f occupies [f, f + 1) * hop / sr and bin b occupies [(b - 1/2) df, (b + 1/2) df), df = sr / (fft_size * zeropad): the
    frame int(t * sr / hop) and the bin round(f / df) the trackers use for a marker (util/wow_detection.py:81-85)."""

    ARGS = ("n", "sr", "fft_size", "hop", "zeropad", "width", "height", "t0", "t1", "f0", "f1", "scale")

    def __init__(self, **kw):
        for k in self.ARGS:
            setattr(self, k, kw[k])
        self.n_frames = stft_frames(self.n, self.fft_size, self.hop)
        self.bins = self.fft_size * self.zeropad // 2 + 1
        self.df = self.sr / (self.fft_size * self.zeropad)
        e = _snap(self._col_edge(np.arange(self.width + 1, dtype=np.float64)))
        fl = np.floor(e)
        lo, hi = fl[:-1], np.maximum(fl[:-1] + 1, fl[1:])
        self.col_lo = np.clip(lo, 0, self.n_frames).astype(np.int64)
        self.col_hi = np.clip(hi, 0, self.n_frames).astype(np.int64)
        g = self._row_edge(np.arange(self.height + 1, dtype=np.float64)) / self.df        # descending: edge 0 is the top
        fl = np.floor(g + 0.5)
        lo, hi = fl[1:], np.maximum(fl[1:] + 1, fl[:-1])
        self.row_lo = np.clip(lo, 0, self.bins).astype(np.int32)
        self.row_hi = np.clip(hi, 0, self.bins).astype(np.int32)
        same = (self.col_lo[1:] == self.col_lo[:-1]) & (self.col_hi[1:] == self.col_hi[:-1])
        if not np.all(same | (self.col_lo[1:] >= self.col_hi[:-1])):
            raise ValueError("column ranges overlap without being equal (a column width within rounding of one frame): move t0 or t1")
        self._dev = {}

    def _col_edge(self, c):
        """left edge of column c in frames, float64: (t0 + (t1 - t0) c / width) sr / hop"""
        return (self.t0 + (self.t1 - self.t0) * c / self.width) * self.sr / self.hop

    def _row_edge(self, r):
        """top edge of row r in Hz: equidistant in the scale's unit from Y(f1) (r = 0) down to Y(f0) (r = height)"""
        y1, y0 = float(_scale_fwd(self.scale, self.f1)), float(_scale_fwd(self.scale, self.f0))
        f = _scale_inv(self.scale, y1 - (y1 - y0) * np.asarray(r, dtype=np.float64) / self.height)
        return np.where(np.asarray(r) == 0, self.f1, np.where(np.asarray(r) == self.height, self.f0, f))

    def args(self):
        """The arguments of geometry() that rebuild this object (what render_file writes beside the picture)"""
        return {k: getattr(self, k) for k in self.ARGS}

    def to_time_freq(self, x, y):
        """(s, Hz) of pixel (x, y): its left edge in time and its LOWER edge in frequency, the corner from which the trackers'
        floor (frame) and round (bin) land inside the pixel's own ranges.  Fractions move right and down the picture."""
        return self._time_of(float(x)), float(self._row_edge(float(y) + 1.0))

    def _time_of(self, x):
        """t0 + (t1 - t0) x / width, moved up by the few ulps it takes for int(t sr / hop) to reach the frame a snapped edge names"""
        t = self.t0 + (self.t1 - self.t0) * x / self.width
        k = float(_snap(t * self.sr / self.hop))
        while k == np.rint(k) and t * self.sr / self.hop < k:
            t = float(np.nextafter(t, np.inf))
        return t

    def to_pixel(self, t, f):
        """The pixel (x, y) that shows what the trackers make of (t, f): frame int(t sr / hop) and bin round(f / df).  Where
        several pixels show that cell (a magnified view) the one (t, f) lies in geometrically; None for a coordinate no pixel
        shows."""
        return self._locate(t, f)

    def _locate(self, t, f):
        frame = int(np.floor(t * self.sr / self.hop))
        b = int(np.floor(f / self.df + 0.5))
        dt = self.t1 - self.t0
        xg = int(np.floor((t - self.t0) / dt * self.width))
        while xg + 1 <= self.width and self.t0 + dt * (xg + 1) / self.width <= t:          # (t - t0) / dt * width rounds either way
            xg += 1
        while xg >= 0 and self.t0 + dt * xg / self.width > t:
            xg -= 1
        x = self._pick(self.col_lo, self.col_hi, frame, xg, ascending=True)
        y1, y0 = float(_scale_fwd(self.scale, self.f1)), float(_scale_fwd(self.scale, self.f0))
        yf = float(_scale_fwd(self.scale, f)) if (f > 0 or self.scale == "linear") else -np.inf
        yg = int(np.ceil((y1 - yf) / (y1 - y0) * self.height)) - 1 if np.isfinite(yf) else self.height
        while 0 <= yg < self.height and self._row_edge(yg + 1.0) > f:
            yg += 1
        while 0 < yg <= self.height and self._row_edge(float(yg)) <= f:
            yg -= 1
        y = self._pick(self.row_lo, self.row_hi, b, yg, ascending=False)
        return None if x is None or y is None else (x, y)

    @staticmethod
    def _pick(lo, hi, cell, guess, ascending):
        if 0 <= guess < len(lo) and lo[guess] <= cell < hi[guess]:
            return int(guess)
        hit = np.flatnonzero((lo <= cell) & (cell < hi))
        if hit.size == 0:
            return None
        return int(hit[np.argmin(np.abs(hit - guess))])

    def col_times(self):
        """left edge of every column in seconds, float64[width]"""
        return np.array([self._time_of(float(c)) for c in range(self.width)], dtype=np.float64)

    def row_freqs(self):
        """lower edge of every row in Hz, float64[height] (descending)"""
        return self._row_edge(np.arange(1, self.height + 1, dtype=np.float64))

    def tables(self):
        """(cols int64[width][2], rows int32[height][2]): the layout the entry points take"""
        return (np.ascontiguousarray(np.stack([self.col_lo, self.col_hi], axis=1)),
                np.ascontiguousarray(np.stack([self.row_lo, self.row_hi], axis=1)))

    def tables_dev(self, dev):
        """tables() on the host and on the device, uploaded once per device"""
        if dev not in self._dev:
            cols, rows = self.tables()
            self._dev[dev] = (cols, rows, torch.from_numpy(cols).to(f"cuda:{dev}"), torch.from_numpy(rows).to(f"cuda:{dev}"))
        return self._dev[dev]


def geometry(n, sr, fft_size, hop, zeropad, width, height, t0=None, t1=None, f0=None, f1=None, scale="mel"):
    """The pixel tables of a width x height picture of seconds [t0, t1) and Hz [f0, f1) of an n-sample signal.
    Defaults: the whole file (t1 = n_frames * hop / sr) and 0 .. sr / 2.  scale: "mel", "linear" or "log" (f0 > 0)."""
    n, fft_size, hop, zeropad, width, height = int(n), int(fft_size), int(hop), int(zeropad), int(width), int(height)
    if scale not in SCALES:
        raise ValueError(f"scale {scale!r}: one of {SCALES}")
    if n < 1 or fft_size < 2 or hop < 1 or zeropad < 1 or not (1 <= width <= _lib.IMAGE_MAX_SIDE and 1 <= height <= _lib.IMAGE_MAX_SIDE):
        raise ValueError(f"geometry: bad sizes (n {n}, fft {fft_size}, hop {hop}, zeropad {zeropad}, image {width} x {height})")
    sr = float(sr)
    t0 = 0.0 if t0 is None else float(t0)
    t1 = stft_frames(n, fft_size, hop) * hop / sr if t1 is None else float(t1)
    f0 = 0.0 if f0 is None else float(f0)
    f1 = sr / 2 if f1 is None else float(f1)
    if not (np.isfinite([t0, t1, f0, f1]).all() and t0 < t1 and 0 <= f0 < f1 and sr > 0):
        raise ValueError(f"geometry: need t0 < t1 and 0 <= f0 < f1 (got {t0}, {t1}, {f0}, {f1})")
    if scale == "log" and f0 <= 0:
        raise ValueError("geometry: the log scale needs f0 > 0")
    return ImageGeometry(n=n, sr=sr, fft_size=fft_size, hop=hop, zeropad=zeropad, width=width, height=height, t0=t0, t1=t1, f0=f0,
                         f1=f1, scale=scale)


def _channel_view(sig_t, channel):
    """-> (1-D float32 view of the channel, element stride, samples)"""
    if sig_t.dtype != torch.float32:
        sig_t = sig_t.to(torch.float32)
    if sig_t.ndim == 1:
        if channel != 0:
            raise ValueError(f"channel {channel} of a one-channel signal")
        sig_t = sig_t.contiguous()
        return sig_t, 1, sig_t.shape[0]
    sig_t = sig_t.contiguous()
    n, ch = sig_t.shape
    if not 0 <= channel < ch:
        raise ValueError(f"channel {channel} of a {ch}-channel signal")
    return sig_t.view(-1)[channel:], ch, n


def peak_image_dev(sig_t, sr, geometry, window_name="blackmanharris", channel=0, fused=None, max_bytes=1 << 30):
    """The peak-hold image of one channel of sig_t (float32 device tensor, (n,) or interleaved (n, channels)) -> device float32
    (width, height): cell [c, r] is the largest float32 magnitude fourier.get_mag holds over the column's frames and the row's
    bins, 0 where there is none.  fused (default FUSED) takes par_stft_peak_image_f32 where fused_supported(); otherwise magnitude
    chunks of at most max_bytes and par_peak_image_f32.  Both give the same bits."""
    g = geometry
    dev = _dev.device_index(sig_t.device)
    x, stride, n = _channel_view(sig_t, channel)
    if n != g.n or float(sr) != g.sr:
        raise ValueError(f"the geometry was made for {g.n} samples at {g.sr} Hz, the signal has {n} at {sr}")
    window_t = fourier.window_dev(window_name, g.fft_size, dev)
    if (FUSED if fused is None else fused) and fused_supported(g.fft_size, g.zeropad):
        return _peak_fused_dev(x, stride, n, g, window_t, dev)
    return _peak_composed_dev(x, stride, n, g, window_t, dev, max_bytes)


def _peak_fused_dev(x, stride, n, g, window_t, dev):
    L = _lib.lib()
    cols, rows, cols_t, rows_t = g.tables_dev(dev)
    peak = _dev.empty((g.width, g.height), torch.float32, dev)
    nbytes = int(L.par_stft_peak_image_scratch_bytes(g.width))
    scratch = _dev.empty(nbytes, torch.uint8, dev)
    _lib.check(L.par_stft_peak_image_f32(dev, _dev.ptr(x), n, stride, g.fft_size, g.hop, g.zeropad, _dev.ptr(window_t), _dev.ptr(cols_t),
                                         cols.ctypes.data, _dev.ptr(rows_t), rows.ctypes.data, g.width, g.height, _dev.ptr(peak), g.height,
                                         _dev.ptr(scratch), nbytes, _dev.stream_ptr(dev)))
    return peak


def _peak_composed_dev(x, stride, n, g, window_t, dev, max_bytes):
    """Stored magnitude chunks of the frames the picture names (spectrum_flat.mag_chunks_dev's framing: a chunk is the STFT of
    the stretch of signal its frames need, begun a few frames early where the reflect padding would differ) maximised into the
    zero-filled image"""
    L = _lib.lib()
    cols, rows, cols_t, rows_t = g.tables_dev(dev)
    peak = torch.zeros((g.width, g.height), dtype=torch.float32, device=f"cuda:{dev}")
    named = g.col_hi > g.col_lo
    if not named.any():
        return peak
    first, last = int(g.col_lo[named].min()), int(g.col_hi[named].max())
    M = g.fft_size * g.zeropad
    per_frame = 4 * g.bins + (8 * M if M > 16384 else 0)
    chunk = max(1, int(max_bytes) // per_frame)
    half = g.fft_size // 2
    lead_max = -(-half // g.hop)
    for fa in range(first, last, chunk):
        fb = min(last, fa + chunk)
        s = max(0, fa - lead_max)
        n_sub = n - s * g.hop
        if fb < g.n_frames:
            n_sub = min(n_sub, (fb - 1 - s) * g.hop + g.fft_size - half)
        mag = fourier.stft_dev(x[s * g.hop * stride:], g.fft_size, g.hop, window_t, g.zeropad, 1, x_stride=stride, n=n_sub, dev=dev)
        fm = mag.T[fa - s:fb - s]
        _lib.check(L.par_peak_image_f32(dev, _dev.ptr(fm), fm.stride(0), g.bins, g.n_frames, fa, fb - fa, _dev.ptr(cols_t),
                                        cols.ctypes.data, _dev.ptr(rows_t), rows.ctypes.data, g.width, g.height, _dev.ptr(peak),
                                        g.height, _dev.stream_ptr(dev)))
    return peak


def peak_image(signal, sr, geometry, window_name="blackmanharris", channel=0, fused=None, max_bytes=1 << 30):
    """peak_image_dev for a numpy signal ((n,) or (n, channels)) -> numpy float32 (width, height)"""
    dev = _dev.device_index(None)
    sig_t = _dev.to_dev(np.asarray(signal), torch.float32, dev)
    return _dev.to_host(peak_image_dev(sig_t, sr, geometry, window_name, channel, fused, max_bytes))


# a handful of RGB knots per built-in map, interpolated linearly to 256 entries
_KNOTS = {
    "gray": ((0.0, (0, 0, 0)), (1.0, (255, 255, 255))),
    "heat": ((0.0, (0, 0, 0)), (0.2, (40, 0, 90)), (0.45, (170, 20, 60)), (0.7, (240, 120, 10)), (0.9, (255, 220, 80)),
             (1.0, (255, 255, 255))),
}


def colormap(name_or_array):
    """-> (256, 4) uint8 RGBA table: "gray" or "heat", a matplotlib name where matplotlib imports, or an array of 256 rows of
    3 or 4 values (floats in 0..1 or integers in 0..255)"""
    if isinstance(name_or_array, str):
        knots = _KNOTS.get(name_or_array)
        if knots is not None:
            pos = np.array([k[0] for k in knots])
            rgb = np.array([k[1] for k in knots], dtype=np.float64)
            t = np.linspace(0.0, 1.0, 256)
            lut = np.stack([np.interp(t, pos, rgb[:, c]) for c in range(3)] + [np.full(256, 255.0)], axis=1)
            return np.floor(lut + 0.5).astype(np.uint8)
        try:
            import matplotlib
            cm = matplotlib.colormaps[name_or_array]
        except (ImportError, KeyError):
            raise ValueError(f"colour map {name_or_array!r}: not built in ({sorted(_KNOTS)}) and not a matplotlib name here") from None
        return np.floor(np.asarray(cm(np.linspace(0.0, 1.0, 256))) * 255.0 + 0.5).astype(np.uint8)
    a = np.asarray(name_or_array)
    if a.ndim != 2 or a.shape[0] != 256 or a.shape[1] not in (3, 4):
        raise ValueError(f"a colour map is (256, 3) or (256, 4), not {a.shape}")
    if a.dtype.kind == "f":
        a = np.floor(np.clip(a, 0.0, 1.0) * 255.0 + 0.5)
    a = a.astype(np.uint8)
    if a.shape[1] == 3:
        a = np.concatenate([a, np.full((256, 1), 255, dtype=np.uint8)], axis=1)
    return np.ascontiguousarray(a)


def colorize_dev(peak_t, vmin=VMIN, vmax=VMAX, cmap="heat"):
    """Device float32 (width, height) peak image -> device uint8 (height, width, 4): lut[floor(clip((dB - vmin) / (vmax - vmin),
    0, 1) * 255 + 0.5)] of dB = 20 log10(peak) in float64; a cell without data (0) or NaN is (0, 0, 0, 0)."""
    dev = _dev.device_index(peak_t.device)
    if peak_t.ndim != 2 or peak_t.dtype != torch.float32:
        raise ValueError("colorize_dev takes a float32 (width, height) image")
    if not vmin < vmax:
        raise ValueError(f"colour limits [{vmin}, {vmax}] are not an interval")
    peak_t = peak_t.contiguous()
    width, height = peak_t.shape
    lut_t = torch.from_numpy(colormap(cmap)).to(f"cuda:{dev}")
    out = _dev.empty((height, width, 4), torch.uint8, dev)
    _lib.check(_lib.lib().par_image_colorize_u8(dev, _dev.ptr(peak_t), width, height, height, float(vmin), float(vmax), _dev.ptr(lut_t),
                                                _dev.ptr(out), _dev.stream_ptr(dev)))
    return out


def colorize(peak, vmin=VMIN, vmax=VMAX, cmap="heat"):
    """colorize_dev for a numpy (width, height) image -> numpy uint8 (height, width, 4)"""
    dev = _dev.device_index(None)
    return _dev.to_host(colorize_dev(_dev.to_dev(np.asarray(peak, dtype=np.float32), torch.float32, dev), vmin, vmax, cmap))


def render(signal, sr, width=2048, height=1024, fft_size=4096, overlap=8, zeropad=1, t0=None, t1=None, f0=None, f1=None, scale="mel",
           vmin=VMIN, vmax=VMAX, cmap="heat", channel=0):
    """signal ((n,) or (n, channels), numpy or device tensor) -> (rgba uint8 (height, width, 4), ImageGeometry); hop = fft_size
    // overlap"""
    dev = _dev.device_index(signal.device if isinstance(signal, torch.Tensor) else None)
    sig_t = _dev.to_dev(signal if isinstance(signal, torch.Tensor) else np.asarray(signal), torch.float32, dev)
    geo = geometry(sig_t.shape[0], sr, fft_size, max(1, int(fft_size) // int(overlap)), zeropad, width, height, t0, t1, f0, f1, scale)
    peak = peak_image_dev(sig_t, sr, geo, channel=channel)
    return _dev.to_host(colorize_dev(peak, vmin, vmax, cmap)), geo


def write_png(path, rgba):
    """(height, width, 4) uint8 -> an RGBA8 PNG, filter 0 on every line, through zlib alone"""
    rgba = np.ascontiguousarray(rgba)
    if rgba.ndim != 3 or rgba.shape[2] != 4 or rgba.dtype != np.uint8 or rgba.shape[0] < 1 or rgba.shape[1] < 1:
        raise ValueError("write_png takes a (height, width, 4) uint8 array")
    height, width = rgba.shape[:2]
    lines = np.zeros((height, 1 + width * 4), dtype=np.uint8)
    lines[:, 1:] = rgba.reshape(height, width * 4)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as out:
        out.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 6, 0, 0, 0)) +
                  chunk(b"IDAT", zlib.compress(lines.tobytes(), 6)) + chunk(b"IEND", b""))


def load_geometry(path):
    """The ImageGeometry of a <stem>_spec.json written by render_file"""
    with open(path) as f:
        return geometry(**json.load(f)["geometry"])


def render_file(path, out=None, signal_data=None, **kw):
    """Audio file -> <stem>_spec.png (or `out`) and, beside it, <that stem>.json with the geometry's arguments, from which
    load_geometry(...).to_time_freq(x, y) turns a pixel back into (s, Hz).  kw: render's; signal_data: (signal, sr) when the
    caller has read the file already.  -> (png path, json path, geometry)"""
    signal, sr = signal_data if signal_data is not None else io_ops.read_file(path)[:2]
    rgba, geo = render(signal, sr, **kw)
    png = out or f"{os.path.splitext(path)[0]}_spec.png"
    meta = f"{os.path.splitext(png)[0]}.json"
    write_png(png, rgba)
    with open(meta, "w") as f:
        json.dump({"source": os.path.basename(path), "channel": kw.get("channel", 0), "geometry": geo.args()}, f, indent=1)
    return png, meta, geo
