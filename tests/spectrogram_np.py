"""The spectrogram image stated on the host, independently of pyaudiorestoration_amd/spectrogram.py: the pixel tables from their
formulas in float64, the peak-hold image as np.max over the cells of a stored magnitude array, and the colours."""
import math

import numpy as np


def stft_frames(n, n_fft, hop):
    return (n + 2 * (n_fft // 2) - n_fft) // hop + 1


def to_mel(f):
    """util/units.py:42-47"""
    return math.log(f / 700.0 + 1.0) * 1127.0


def scale_fwd(scale, f):
    return {"mel": to_mel, "linear": float, "log": math.log2}[scale](f)


def scale_inv(scale, y):
    return {"mel": lambda v: (math.exp(v / 1127.0) - 1.0) * 700.0, "linear": float, "log": lambda v: 2.0 ** v}[scale](y)


def time_2_frame(t, sr, hop):
    """util/wow_detection.py:84-85"""
    return int(t * sr / hop)


def freq_2_bin(f, fft_size, sr, num_bins):
    """util/wow_detection.py:81-82"""
    return max(1, min(num_bins - 1, int(round(f * fft_size / sr))))


def snap(e):
    """an edge within 1e-9 frames (relative, above one frame) of a whole frame is that frame: the rounding of the float64
    expression (a few 1e-16) must not move an edge that is a whole frame in exact arithmetic under it"""
    k = round(e)
    return float(k) if abs(e - k) <= 1e-9 * max(1.0, abs(e)) else e


def column_tables(n, sr, n_fft, hop, width, t0, t1):
    """(lo, hi) int64[width]: e_c = (t0 + (t1 - t0) c / width) sr / hop; lo = floor(e_c), hi = max(lo + 1, floor(e_{c+1})), both
    clamped to [0, n_frames] -- a Python loop over the columns, one float64 expression each"""
    n_frames = stft_frames(n, n_fft, hop)
    lo, hi = np.zeros(width, dtype=np.int64), np.zeros(width, dtype=np.int64)
    for c in range(width):
        e0 = snap((t0 + (t1 - t0) * c / width) * sr / hop)
        e1 = snap((t0 + (t1 - t0) * (c + 1) / width) * sr / hop)
        a = math.floor(e0)
        b = max(a + 1, math.floor(e1))
        lo[c], hi[c] = min(max(a, 0), n_frames), min(max(b, 0), n_frames)
    return lo, hi


def row_tables(sr, n_fft, zeropad, height, f0, f1, scale):
    """(lo, hi) int32[height], row 0 on top: edges equidistant in the scale's unit from Y(f1) down to Y(f0), in bins g = f / df;
    lo = floor(g_lo + 0.5), hi = max(lo + 1, floor(g_hi + 0.5)), clamped to [0, bins]"""
    bins = n_fft * zeropad // 2 + 1
    df = sr / (n_fft * zeropad)
    y1, y0 = scale_fwd(scale, f1), scale_fwd(scale, f0)

    def edge(r):
        if r == 0:
            return f1
        if r == height:
            return f0
        return scale_inv(scale, y1 - (y1 - y0) * r / height)
    lo, hi = np.zeros(height, dtype=np.int32), np.zeros(height, dtype=np.int32)
    for r in range(height):
        g_hi, g_lo = edge(r) / df, edge(r + 1) / df
        a = math.floor(g_lo + 0.5)
        b = max(a + 1, math.floor(g_hi + 0.5))
        lo[r], hi[r] = min(max(a, 0), bins), min(max(b, 0), bins)
    return lo, hi


def peak_tables_np(mag, col_lo, col_hi, row_lo, row_hi):
    """mag: float32 [n_frames][bins] (frame-major, as the device stores it) -> float32 (width, height): np.max over every cell, 0.0
    for a cell without a frame or a bin; a NaN in a cell makes it NaN (np.max propagates).  The maximum over a cell is taken as
    the maximum over its bins of the maxima over its frames (np.max both times; a maximum has no order), which lets a column's
    frames be reduced once for all its rows; a row of one bin is that bin's value."""
    row_lo, row_hi = np.asarray(row_lo, dtype=np.int64), np.asarray(row_hi, dtype=np.int64)
    out = np.zeros((len(col_lo), len(row_lo)), dtype=np.float32)
    single = np.flatnonzero(row_hi - row_lo == 1)
    wide = np.flatnonzero(row_hi - row_lo > 1)
    for c in range(len(col_lo)):
        if col_hi[c] <= col_lo[c]:
            continue
        if c > 0 and col_lo[c] == col_lo[c - 1] and col_hi[c] == col_hi[c - 1]:
            out[c] = out[c - 1]
            continue
        over_frames = np.max(mag[col_lo[c]:col_hi[c]], axis=0)
        out[c, single] = over_frames[row_lo[single]]
        for r in wide:
            out[c, r] = np.max(over_frames[row_lo[r]:row_hi[r]])
    return out


def peak_np(mag, geometry):
    return peak_tables_np(mag, geometry.col_lo, geometry.col_hi, geometry.row_lo, geometry.row_hi)


def colorize_t(peak, vmin, vmax):
    """numpy's t * 255 + 0.5 per cell, float64 (NaN where the cell has no data or is NaN)"""
    m = np.asarray(peak, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        dB = 20.0 * np.log10(m)
        t = (dB - vmin) / (vmax - vmin)
    v = np.minimum(np.maximum(t, 0.0), 1.0) * 255.0 + 0.5
    return np.where((m == 0) | np.isnan(m), np.nan, v)


def colorize_np(peak, vmin, vmax, lut):
    """peak float32 (width, height) -> uint8 (height, width, 4)"""
    v = colorize_t(peak, vmin, vmax)
    nodata = np.isnan(v)
    idx = np.floor(np.where(nodata, 0.0, v)).astype(np.int64)
    out = np.asarray(lut, dtype=np.uint8)[idx]
    out[nodata] = 0
    return np.ascontiguousarray(out.transpose(1, 0, 2))


def colorize_seeded_input(count=65536, seed=20260):
    """The random magnitudes of the colorize tests: log-uniform over -130 .. +5 dB, float32"""
    rng = np.random.default_rng(seed)
    return (10.0 ** (rng.uniform(-130.0, 5.0, count) / 20.0)).astype(np.float32)


def png_decode(data):
    """A minimal PNG decoder for what write_png writes: 8-bit RGBA, no interlace, filter 0 on every line"""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        (ln,), tag = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + ln]
        (crc,) = struct.unpack(">I", data[pos + 8 + ln:pos + 12 + ln])
        assert crc == zlib.crc32(tag + body) & 0xffffffff, tag
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + ln
    width, height, depth, colour, comp, filt, lace = hdr
    assert (depth, colour, comp, filt, lace) == (8, 6, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(height, 1 + 4 * width)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(height, width, 4).copy()
