"""Spectrogram image without a GPU: the pixel tables against their float64 statement (tests/spectrogram_np.py), the pixel <->
(s, Hz) maps against the trackers' frame and bin rules, every argument check of the three entry points (all of them return
before a device call), the PNG writer and the colour maps."""
import ctypes
import math
import os

import numpy as np
import pytest

import spectrogram_np as SN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sp():
    from pyaudiorestoration_amd import spectrogram
    return spectrogram


def frames_of(n, fft, hop):
    return SN.stft_frames(n, fft, hop)


def n_for_frames(frames, fft, hop):
    n = (frames - 1) * hop
    assert frames_of(n, fft, hop) == frames
    return n


# ---------------------------------------------------------------------------------------------------------------- columns
@pytest.mark.parametrize("width", [1, 3, 7, 39, 40, 41, 120, 333])
def test_columns_match_the_formula_and_partition_the_frames(sp, width):
    sr, fft, hop, frames = 8000.0, 64, 16, 40
    n = n_for_frames(frames, fft, hop)
    g = sp.geometry(n, sr, fft, hop, 1, width, 5)
    lo, hi = SN.column_tables(n, sr, fft, hop, width, 0.0, frames * hop / sr)
    assert g.n_frames == frames and g.col_lo.dtype == np.int64 and g.col_hi.dtype == np.int64
    assert np.array_equal(g.col_lo, lo) and np.array_equal(g.col_hi, hi)
    if width < frames:                        # decimating: every frame in exactly one column
        count = np.zeros(frames, dtype=int)
        for a, b in zip(lo, hi):
            count[a:b] += 1
        assert np.all(count == 1)
    elif width == frames:                     # the boundary: one to one
        assert np.array_equal(lo, np.arange(frames)) and np.array_equal(hi, np.arange(frames) + 1)
    else:                                     # magnifying: one frame per column, non-decreasing, repeated ranges identical
        assert np.all(hi - lo == 1) and np.all(np.diff(lo) >= 0) and set(lo) == set(range(frames))
    same = (lo[1:] == lo[:-1]) & (hi[1:] == hi[:-1])
    assert np.all(same | (lo[1:] >= hi[:-1]))


@pytest.mark.parametrize("t0,t1", [(-3.0, -1.0), (5.0, 9.0), (-0.02, 0.03), (0.05, 0.2), (-0.05, 0.2), (-1.0, -0.0001)])
def test_columns_outside_the_file_are_empty(sp, t0, t1):
    sr, fft, hop, frames = 8000.0, 64, 16, 40                     # the file is 0.08 s long
    n = n_for_frames(frames, fft, hop)
    for width in (4, 50, 200):
        g = sp.geometry(n, sr, fft, hop, 1, width, 3, t0=t0, t1=t1)
        lo, hi = SN.column_tables(n, sr, fft, hop, width, t0, t1)
        assert np.array_equal(g.col_lo, lo) and np.array_equal(g.col_hi, hi)
        assert np.all((lo >= 0) & (lo <= hi) & (hi <= frames))
        times = g.col_times()
        step = (t1 - t0) / width
        for c in range(width):
            if times[c] + step <= 0 or times[c] >= frames * hop / sr:
                assert lo[c] == hi[c], (c, lo[c], hi[c])
        if t1 <= 0 or t0 >= frames * hop / sr:
            assert np.all(lo == hi)


# ------------------------------------------------------------------------------------------------------------------- rows
@pytest.mark.parametrize("scale", ["mel", "linear", "log"])
@pytest.mark.parametrize("fft,zp", [(64, 1), (256, 2)])
def test_rows_match_the_formula_cover_the_band_and_stay_small(sp, scale, fft, zp):
    sr, hop = 44100.0, 16
    bins = fft * zp // 2 + 1
    for height in (1, 7, bins, 2 * bins):
        for f0, f1 in ((None, None), (300.0, 9000.0), (20.0, 30000.0)):
            if scale == "log" and f0 is None:
                with pytest.raises(ValueError):
                    sp.geometry(1000, sr, fft, hop, zp, 4, height, f0=f0, f1=f1, scale=scale)
                continue
            g = sp.geometry(1000, sr, fft, hop, zp, 4, height, f0=f0, f1=f1, scale=scale)
            lo, hi = SN.row_tables(sr, fft, zp, height, g.f0, g.f1, scale)
            assert g.row_lo.dtype == np.int32 and np.array_equal(g.row_lo, lo) and np.array_equal(g.row_hi, hi)
            assert np.all((lo >= 0) & (lo <= hi) & (hi <= bins))
            if g.f1 <= sr / 2:
                assert np.all(hi > lo)                                     # non-empty inside the band
            assert np.all(np.diff(lo) <= 0) and np.all(np.diff(hi) <= 0)     # monotone: row 0 is the top
            seen = np.zeros(bins + 1, dtype=bool)
            for a, b in zip(lo, hi):
                seen[a:b] = True
            shown = np.flatnonzero(seen)
            assert np.all(seen[shown[0]:shown[-1] + 1])                    # the union has no hole
            assert int(np.sum(hi - lo)) <= bins + height


def test_mel_constants(sp):
    assert SN.to_mel(1000.0) == math.log(1000.0 / 700.0 + 1.0) * 1127.0
    assert abs(SN.to_mel(1000.0) - 1000.0) < 0.01                          # the constants put 1000 Hz on 1000 mel (999.9907)
    from pyaudiorestoration_amd.spectrogram import _scale_fwd, _scale_inv
    assert float(_scale_fwd("mel", 1000.0)) == pytest.approx(SN.to_mel(1000.0), rel=1e-15)
    assert float(_scale_inv("mel", _scale_fwd("mel", 1234.5))) == pytest.approx(1234.5, rel=1e-13)


# ------------------------------------------------------------------------------------------------------------ pixel maps
@pytest.mark.parametrize("scale", ["mel", "linear", "log"])
@pytest.mark.parametrize("width,height", [(13, 9), (40, 33), (90, 70)])
def test_pixels_land_on_the_trackers_frame_and_bin(sp, scale, width, height):
    """(t, f) = to_time_freq(x, y) gives the frame int(t sr / hop) and the bin round(f fft / sr) of util/wow_detection.py:81-85
    inside the pixel's own ranges, and to_pixel takes (t, f) back to (x, y)"""
    sr, fft, hop, frames = 8000.0, 64, 16, 40
    n = n_for_frames(frames, fft, hop)
    bins = fft // 2 + 1
    g = sp.geometry(n, sr, fft, hop, 1, width, height, f0=150.0, f1=3900.0, scale=scale)
    assert len(g.col_times()) == width and len(g.row_freqs()) == height
    for x in range(width):
        for y in range(height):
            t, f = g.to_time_freq(x, y)
            assert t == g.col_times()[x] and f == g.row_freqs()[y]
            fr = SN.time_2_frame(t, sr, hop)
            assert g.col_lo[x] <= fr < g.col_hi[x], (x, t, fr)
            g_bins = f * fft / sr
            if abs(g_bins + 0.5 - round(g_bins + 0.5)) > 1e-9:             # (Python rounds a tie to even, the tables floor it)
                b = SN.freq_2_bin(f, fft, sr, bins)
                assert g.row_lo[y] <= b < g.row_hi[y], (y, f, b)
                assert g.to_pixel(t, f) == (x, y)
    assert g.to_pixel(-1.0, 1000.0) is None and g.to_pixel(0.01, 10.0) is None


def test_geometry_arguments_round_trip_and_are_checked(sp):
    g = sp.geometry(5000, 44100, 256, 32, 2, 31, 17, t0=0.01, t1=0.09, f0=100, f1=8000, scale="log")
    h = sp.geometry(**g.args())
    assert h.args() == g.args() and np.array_equal(h.col_lo, g.col_lo) and np.array_equal(h.row_hi, g.row_hi)
    cols, rows = g.tables()
    assert cols.shape == (31, 2) and cols.dtype == np.int64 and rows.shape == (17, 2) and rows.dtype == np.int32
    for bad in (dict(t0=1.0, t1=1.0), dict(f0=500.0, f1=400.0), dict(scale="bark"), dict(width=0), dict(f0=-1.0)):
        with pytest.raises(ValueError):
            sp.geometry(**dict(g.args(), **bad))
    assert sp.fused_supported(4096, 4) and not sp.fused_supported(4096, 8) and not sp.fused_supported(1000, 1)
    assert sp.fused_supported(16, 1) and not sp.fused_supported(8, 1)


# ------------------------------------------------------------------------------------------------------- argument checks
P = ctypes.c_void_p(64)       # a non-null pointer no check dereferences


def _tables(cols, rows):
    c = np.ascontiguousarray(np.asarray(cols, dtype=np.int64).reshape(-1, 2))
    r = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 2))
    return c, r


def _fused(L, **kw):
    a = dict(x=P, n=1000, x_stride=1, n_fft=64, hop=16, zeropad=1, window=P, cols=P, cols_host=None, rows=P, rows_host=None, width=None,
             height=None, peak=P, pitch=None, scratch=P, scratch_bytes=1 << 20)
    c, r = _tables(kw.pop("cols_tab", [[0, 10], [10, 20]]), kw.pop("rows_tab", [[20, 33], [0, 20]]))
    a.update(cols_host=c.ctypes.data, rows_host=r.ctypes.data, width=len(c), height=len(r), pitch=len(r))
    a.update(kw)
    return L.par_stft_peak_image_f32(0, a["x"], a["n"], a["x_stride"], a["n_fft"], a["hop"], a["zeropad"], a["window"], a["cols"],
                                     a["cols_host"], a["rows"], a["rows_host"], a["width"], a["height"], a["peak"], a["pitch"],
                                     a["scratch"], a["scratch_bytes"], None)


def _composed(L, **kw):
    a = dict(mag=P, mag_pitch=33, bins=33, n_frames=63, frame_first=0, n_frames_chunk=10, cols=P, rows=P, peak=P)
    c, r = _tables(kw.pop("cols_tab", [[0, 10], [10, 20]]), kw.pop("rows_tab", [[20, 33], [0, 20]]))
    a.update(cols_host=c.ctypes.data, rows_host=r.ctypes.data, width=len(c), height=len(r), pitch=len(r))
    a.update(kw)
    return L.par_peak_image_f32(0, a["mag"], a["mag_pitch"], a["bins"], a["n_frames"], a["frame_first"], a["n_frames_chunk"], a["cols"],
                                a["cols_host"], a["rows"], a["rows_host"], a["width"], a["height"], a["peak"], a["pitch"], None)


def test_fused_entry_point_rejects_bad_arguments_before_any_device_call():
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    ARG, UNSUPPORTED, WORKSPACE = 1, 3, 4
    assert L.par_stft_frames(1000, 64, 16) == 63
    for name in ("x", "window", "cols", "cols_host", "rows", "rows_host", "peak", "scratch"):
        assert _fused(L, **{name: None}) == ARG and "null" in _lib.last_error(), name
    for name in ("n", "hop", "zeropad", "x_stride", "width", "height"):
        assert _fused(L, **{name: 0}) == ARG and "bad sizes" in _lib.last_error(), name
    assert _fused(L, pitch=1) == ARG and "bad sizes" in _lib.last_error()
    assert _fused(L, width=_lib.IMAGE_MAX_SIDE + 1) == ARG
    assert _fused(L, scratch=ctypes.c_void_p(68)) == ARG and "aligned" in _lib.last_error()
    # sizes the register path does not take
    for n_fft, zp in ((8, 1), (100, 1), (64, 3), (4096, 8), (32768, 1), (6, 8)):
        assert _fused(L, n_fft=n_fft, zeropad=zp) == UNSUPPORTED and "power of two" in _lib.last_error(), (n_fft, zp)
    with pytest.raises(_lib.ParUnsupported):
        _lib.check(_fused(L, n_fft=32768))
    # column tables: outside [0, n_frames], lo > hi, overlapping, descending
    for cols in ([[-1, 3]], [[0, 64]], [[5, 4]], [[0, 10], [9, 20]], [[10, 20], [0, 10]], [[0, 10], [0, 11]], [[0, 10], [1, 10]]):
        assert _fused(L, cols_tab=cols) == ARG and "column" in _lib.last_error(), cols
    # ... and what is legal: empty columns, repeats, gaps -- they get as far as the workspace check
    for cols in ([[0, 0], [0, 3], [3, 3]], [[4, 5], [4, 5], [4, 5], [5, 6]], [[0, 2], [40, 63], [63, 63]]):
        assert _fused(L, cols_tab=cols, scratch_bytes=0) == WORKSPACE, cols
    # row tables: outside [0, bins], lo > hi, too many bins named
    for rows in ([[-1, 3]], [[0, 34]], [[7, 6]]):
        assert _fused(L, rows_tab=rows) == ARG and "row" in _lib.last_error(), rows
    assert _fused(L, rows_tab=[[0, 33], [0, 33]]) == ARG and "more than bins + height" in _lib.last_error()
    assert _fused(L, rows_tab=[[0, 33], [31, 33]], scratch_bytes=0) == WORKSPACE                 # 35 = bins + height: the limit
    assert _fused(L, rows_tab=[[3, 9], [20, 33], [0, 0], [9, 20]], scratch_bytes=0) == WORKSPACE   # any order, empty rows
    # workspace
    assert L.par_stft_peak_image_scratch_bytes(2) == 24 and L.par_stft_peak_image_scratch_bytes(0) == 0
    assert _fused(L, scratch_bytes=23) == WORKSPACE and "scratch" in _lib.last_error()


def test_composed_and_colorize_entry_points_reject_bad_arguments_before_any_device_call():
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    ARG = 1
    for name in ("mag", "cols", "cols_host", "rows", "rows_host", "peak"):
        assert _composed(L, **{name: None}) == ARG and "null" in _lib.last_error(), name
    for kw in (dict(bins=0), dict(mag_pitch=32), dict(width=0), dict(height=0), dict(pitch=1), dict(frame_first=-1), dict(n_frames_chunk=-1),
               dict(frame_first=60, n_frames_chunk=4), dict(n_frames_chunk=64)):
        assert _composed(L, **kw) == ARG and "bad sizes" in _lib.last_error(), kw
    assert _composed(L, cols_tab=[[0, 10], [9, 20]]) == ARG and "column" in _lib.last_error()
    assert _composed(L, rows_tab=[[0, 34]]) == ARG and "row" in _lib.last_error()
    assert _composed(L, n_frames_chunk=0) == 0                                                   # nothing to do, no device call

    def colour(**kw):
        a = dict(peak=P, width=4, height=3, pitch=3, vmin=-120.0, vmax=0.0, lut=P, out=P)
        a.update(kw)
        return L.par_image_colorize_u8(0, a["peak"], a["width"], a["height"], a["pitch"], a["vmin"], a["vmax"], a["lut"], a["out"], None)
    for name in ("peak", "lut", "out"):
        assert colour(**{name: None}) == ARG and "null" in _lib.last_error(), name
    for kw in (dict(width=0), dict(height=0), dict(pitch=2)):
        assert colour(**kw) == ARG and "bad sizes" in _lib.last_error(), kw
    for kw in (dict(vmin=0.0, vmax=0.0), dict(vmin=1.0, vmax=0.0), dict(vmin=float("nan")), dict(vmax=float("inf"))):
        assert colour(**kw) == ARG and "interval" in _lib.last_error(), kw
    assert colour(lut=ctypes.c_void_p(66)) == ARG and "aligned" in _lib.last_error()


def test_geometry_tables_pass_the_entry_points_checks(sp):
    """the tables geometry() makes are tables the entry points take: they reach the workspace check"""
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    n = 1000
    for width, height, kw in ((1, 1, {}), (200, 66, {}), (63, 33, dict(scale="linear")), (17, 40, dict(t0=-0.05, t1=0.3, f0=50, scale="log"))):
        g = sp.geometry(n, 8000, 64, 16, 1, width, height, **kw)
        cols, rows = g.tables()
        assert _fused(L, n=n, cols_tab=cols, rows_tab=rows, scratch_bytes=0) == 4, (width, height)      # PAR_ERR_WORKSPACE


# ------------------------------------------------------------------------------------------------------- PNG and colours
def test_write_png_round_trips(sp, tmp_path):
    rng = np.random.default_rng(5)
    for shape in ((1, 1, 4), (7, 13, 4), (64, 200, 4)):
        rgba = rng.integers(0, 256, shape, dtype=np.uint8)
        path = str(tmp_path / f"p{shape[0]}.png")
        sp.write_png(path, rgba)
        assert np.array_equal(SN.png_decode(open(path, "rb").read()), rgba)
        try:
            from PIL import Image
        except ImportError:
            continue
        with Image.open(path) as im:
            assert im.mode == "RGBA" and np.array_equal(np.asarray(im), rgba)
    with pytest.raises(ValueError):
        sp.write_png(str(tmp_path / "bad.png"), np.zeros((4, 4, 3), dtype=np.uint8))


def test_colormaps(sp):
    for name in ("gray", "heat"):
        lut = sp.colormap(name)
        assert lut.shape == (256, 4) and lut.dtype == np.uint8 and np.all(lut[:, 3] == 255)
    gray = sp.colormap("gray").astype(int)
    assert np.array_equal(gray[:, 0], np.arange(256)) and np.all(np.diff(gray[:, :3].sum(axis=1)) > 0)
    heat = sp.colormap("heat").astype(float)
    lum = heat[:, :3] @ np.array([0.2126, 0.7152, 0.0722])
    assert np.all(np.diff(lum) >= 0) and tuple(heat[0, :3]) == (0, 0, 0) and tuple(heat[255, :3]) == (255, 255, 255)
    user = np.linspace(0, 1, 256)[:, None] * np.ones((1, 3))
    assert np.array_equal(sp.colormap(user), sp.colormap("gray"))
    u8 = np.arange(1024, dtype=np.uint8).reshape(256, 4)
    assert np.array_equal(sp.colormap(u8), u8)
    with pytest.raises(ValueError):
        sp.colormap(np.zeros((10, 3)))
    with pytest.raises(ValueError):
        sp.colormap("no such colour map")
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    assert sp.colormap("viridis").shape == (256, 4)


def test_colorize_seeded_input_keeps_clear_of_the_rounding_edges():
    """precondition of the GPU colorize test: at most 0.1 % of the seeded magnitudes have t * 255 + 0.5 within 1e-6 of an integer"""
    m = SN.colorize_seeded_input()
    v = SN.colorize_t(m, -120.0, 0.0)
    assert m.shape == (65536,) and m.dtype == np.float32 and not np.isnan(v).any()
    near = np.abs(v - np.rint(v)) < 1e-6
    inside = (v > 0.5) & (v < 255.5)
    assert inside.mean() > 0.8
    assert near[inside].sum() <= 0.001 * m.size
    # (cells clipped to 0 or 1 sit on 0.5 and 255.5 exactly: far from an integer)
    assert not near[~inside].any()
