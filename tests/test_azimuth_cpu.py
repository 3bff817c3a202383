"""Host side of the tape-sync azimuth mode (pytapesynch_gui.py:210-238): window geometry against a literal restatement of
Spectrum.get_signal, AzimuthLine.update_reject, LagLine with azimuth lines against arrays the reference computed
(tests/golden/azimuth.npz, tools/gen_golden_azimuth.py), the preconditions of every input tests/test_azimuth_gpu.py uses --
proved with the float64 oracles alone --, the new entry points' argument errors and the CLI.  Runs without a GPU."""
import ctypes
import json
import os

import numpy as np
import pytest

import azimuth_inputs as A
import xcorr_inputs as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- window geometry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", A.geometry_cases(), ids=lambda g: g.name)
def test_azimuth_windows_equal_get_signal(g):
    """start, length and both pads of every window of both files, and the cut arrays themselves, equal Spectrum.get_signal's"""
    from pyaudiorestoration_amd import pipeline
    ref, src = A.geometry_signals(g)
    times, lags, want = A.windows_of(ref, src, g.sr, g.t0, g.t1, g.lag_curve, g.dur, g.overlap)
    got_t, got_l, ref_geom, src_geom = pipeline.azimuth_windows(g.len_ref, g.len_src, g.sr, g.t0, g.t1, g.lag_curve, g.dur, g.overlap)
    assert np.array_equal(got_t, times) and np.array_equal(got_l, lags)
    assert ref_geom.shape == src_geom.shape == (len(times), 4) and ref_geom.dtype == np.int64
    if g.name.startswith("empty"):
        assert len(times) == 0
        return
    assert len(times) >= 4
    for i, (a, b, ga, gb) in enumerate(want):
        assert tuple(ref_geom[i]) == ga and tuple(src_geom[i]) == gb, (g.name, i, ref_geom[i], ga, src_geom[i], gb)
        for sig, (start, length, pad_l, pad_r), cut in ((ref, ref_geom[i], a), (src, src_geom[i], b)):
            assert start >= 0 and length >= 0 and start + length <= len(sig)
            mine = np.concatenate((np.zeros(pad_l, sig.dtype), sig[start:start + length], np.zeros(pad_r, sig.dtype)))
            assert np.array_equal(mine, cut), (g.name, i)
    # the case is what its name says
    s0 = lambda geom: geom[:, 2]
    if g.name == "inside":
        assert not ref_geom[:, 2:].any() and not src_geom[:, 2:].any()
        assert len({(int(a[1]), int(b[1])) for a, b in zip(ref_geom, src_geom)}) >= 2          # lengths differ by a sample
    if g.name == "over_the_end":
        assert ref_geom[-1, 3] > 0 and src_geom[-1, 3] > 0 and ref_geom[0, 3] == 0
    if g.name == "before_0_ref_only":
        assert s0(ref_geom)[0] > 0 and not s0(src_geom).any()
    if g.name == "before_0_src_only":
        assert s0(src_geom)[0] > 0 and not s0(ref_geom).any()
    if g.name == "before_0_both":
        assert s0(ref_geom)[0] > 0 and s0(src_geom)[0] > 0
    if g.name == "int_truncates_from_below":
        assert (g.t0 - g.dur) * g.sr < 0 and int((g.t0 - g.dur) * g.sr) == 0 and tuple(ref_geom[0, :3]) == (0, 799, 0)
    if g.name == "src_past_the_end":
        assert np.all(src_geom[:, 1] == 0) and np.all(src_geom[:, 3] > 800)
    if g.name == "src_before_the_start":                          # both indices negative but inside -len: Python counts from the END
        assert np.all(src_geom[:, 1] >= 799) and np.all(src_geom[:, 2] > 800) and np.all(src_geom[:, 0] > 0)
    if g.name == "src_far_before_the_start":
        assert np.all(src_geom[:, 1] == 0) and np.all(src_geom[:, 2] > g.len_src)
    if g.name == "short_file":
        assert ref_geom[0, 1] > 0 and ref_geom[0, 2] > 0 and ref_geom[0, 0] > 0       # Python's negative start: a slice from the END


def test_times_freqs_clamps_like_get_times_freqs():
    from pyaudiorestoration_amd import pipeline
    assert pipeline.times_freqs((2.0, 0.2), (1.0, 30000.0), 44100) == (1.0, 2.0, 1, 22049)
    assert pipeline.times_freqs((1.0, 500.0), (2.0, 300.0), 8000) == (1.0, 2.0, 300.0, 500.0)


# ---- azimuth_reject ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [4, 5, 32])
def test_azimuth_reject_equals_update_reject(overlap):
    from pyaudiorestoration_amd import pipeline
    rng = np.random.default_rng(83)
    n = 61
    lags = 0.003 + 1e-4 * rng.standard_normal(n)
    lags[7] += 0.01                                               # an outlier for the median
    corrs = rng.uniform(0.2, 0.9, n) * rng.choice([-1.0, 1.0], n)
    for lo, hi in ((20, 29), (0, 3), (n - 4, n), (0, 0)):
        c = corrs.copy()
        c[lo:hi] = 0.05 * np.sign(c[lo:hi])
        keep_l, keep_c = lags.copy(), c.copy()
        got = pipeline.azimuth_reject(lags, c, overlap, A.REJECT)
        assert np.array_equal(got, A.reject_np(lags, c, overlap, A.REJECT)), (overlap, lo, hi)
        assert np.array_equal(lags, keep_l) and np.array_equal(c, keep_c)      # the raw data is not touched
    c = corrs.copy()
    c[3] = np.nan                                                 # a window of silence: NaN corr is NOT below reject, its NaN lag is filled
    l2 = lags.copy()
    l2[3] = np.nan
    assert np.array_equal(pipeline.azimuth_reject(l2, c, overlap, A.REJECT), A.reject_np(l2, c, overlap, A.REJECT))
    dead = pipeline.azimuth_reject(lags, np.full(n, 0.01), overlap, A.REJECT)
    assert dead.shape == (n,) and np.all(np.isnan(dead))                       # nothing accepted: all NaN, no exception
    assert pipeline.azimuth_reject(np.zeros(0), np.zeros(0), overlap, A.REJECT).shape == (0,)


# ---- lag_curve_from_markers with azimuth lines -------------------------------------------------------------------------------------
def _tapesync():
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "rhythm.tapesync")))
    return cfg, 44100, cfg["fft_size"] // cfg["fft_overlap"], 1344000 / 44100


def test_lag_curve_default_keyword_changes_nothing():
    from pyaudiorestoration_amd import pipeline
    cfg, sr, hop, dur = _tapesync()
    a = pipeline.lag_curve_from_markers(cfg["markers"], dur, sr, hop, cfg["smoothing"])
    b = pipeline.lag_curve_from_markers(cfg["markers"], dur, sr, hop, cfg["smoothing"], azimuths=())
    assert a.dtype == b.dtype == np.float64 and np.array_equal(a, b)
    assert np.array_equal(a, pipeline.project_lag_curve(cfg, dur, sr))


@pytest.fixture(scope="module")
def az_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "azimuth.npz"))


def test_golden_geometry_reject_and_lag_curve(az_golden):
    """arrays the reference computed on rhythm.flac / rhythm+5percent.flac (tools/gen_golden_azimuth.py): the windows' geometry and the
    rejected lags bit for bit, LagLine's grid bit for bit, its unfiltered samples within 1e-9"""
    from pyaudiorestoration_amd import pipeline
    g = az_golden
    sr, hop = int(g["sr"]), int(g["hop"])
    times, lags, ref_geom, src_geom = pipeline.azimuth_windows(int(g["len_ref"]), int(g["len_src"]), sr, float(g["t0"]), float(g["t1"]),
                                                               g["lag_curve0"], float(g["dur"]), int(g["overlap"]))
    assert np.array_equal(times, g["sample_times"]) and np.array_equal(lags, g["sample_lags"])
    assert np.array_equal(ref_geom, g["ref_geom"]) and np.array_equal(src_geom, g["src_geom"])
    assert np.array_equal(pipeline.azimuth_reject(g["lags_raw"], g["corrs"], int(g["overlap"]), float(g["reject"])), g["lags"])
    cfg, _, _, _ = _tapesync()
    line = (g["sample_times"], g["lags"], g["corrs"], float(g["lower"]), float(g["upper"]))
    curve = pipeline.lag_curve_from_markers(cfg["markers"], float(g["duration"]), sr, hop, int(g["smoothing"]), azimuths=(line,))
    assert curve.shape == (int(g["curve_len"]), 2)
    full, curve, want = curve, curve[g["curve_rows"]], g["curve_unfiltered"]         # the fixture keeps a subset of the rows
    assert np.array_equal(curve[:, 0], want[:, 0])
    assert np.max(np.abs(curve[:, 1] - want[:, 1])) <= 1e-9
    inside = (curve[:, 0] > g["sample_times"][0]) & (curve[:, 0] < g["sample_times"][-1])
    assert inside.sum() >= 3 and np.array_equal(curve[inside, 1], want[inside, 1])       # np.interp into float32: no spline there
    # the project layout ParamWidget.save writes: "lags" and "azimuths"
    new = dict(cfg, lags=cfg["markers"], azimuths=[[list(v) if np.ndim(v) else v for v in line]])
    del new["markers"]
    assert np.array_equal(pipeline.project_lag_curve(new, float(g["duration"]), sr), full)


def test_lag_curve_hand_cases():
    from pyaudiorestoration_amd import pipeline
    sr, hop, dur = 48000, 256, 10.0
    marks = [(1.0, 0, 1.0, 0, 0.010, 0.5), (9.0, 0, 9.0, 0, 0.012, 0.5)]
    plain = pipeline.lag_curve_from_markers(marks, dur, sr, hop)
    l1 = (np.array([2.0, 4.0]), np.array([0.1, 0.3]), np.array([0.5, 0.5]), 100.0, 200.0)
    l2 = (np.array([3.0, 5.0]), np.array([0.2, 0.2]), np.array([0.5, 0.5]), 100.0, 200.0)
    l3 = (np.array([7.0, 8.0]), np.array([0.4, 0.4]), np.array([0.5, 0.5]), 100.0, 200.0)
    got = pipeline.lag_curve_from_markers(marks, dur, sr, hop, azimuths=(l1, pipeline.AzimuthLine(*l2, l2[1]), l3))
    from scipy.interpolate import InterpolatedUnivariateSpline
    t = got[:, 0]
    # the end time: the spline at `duration`, no line reaches it -- through sample_at's float32 array, so to float32's spacing
    assert len(t) == len(plain) and t[0] == 0 and abs(t[-1] - plain[-1, 0]) < 1e-6
    spline = InterpolatedUnivariateSpline([1.0, 9.0], [0.010, 0.012], k=1)(t)
    f32 = lambda v: np.asarray(v, dtype=np.float32)
    s1, s2 = f32(np.interp(t, l1[0], l1[1])), f32(np.interp(t, l2[0], l2[1]))
    both, only1, only2 = (t >= 3.0) & (t <= 4.0), (t >= 2.0) & (t < 3.0), (t > 4.0) & (t <= 5.0)
    assert both.sum() > 100 and np.array_equal(got[both, 1], ((s1 + s2) / np.float32(2))[both])       # nanmean of two float32 columns
    assert np.array_equal(got[only1, 1], s1[only1]) and np.array_equal(got[only2, 1], s2[only2])
    assert np.any(got[only1, 1] != np.interp(t, l1[0], l1[1])[only1])                                 # float32 rounding is visible
    gap = (t > 5.0) & (t < 7.0)                                 # between the lines: the markers' spline, through the float32 array
    assert gap.sum() > 100 and np.array_equal(got[gap, 1], f32(spline[gap]))
    alone = pipeline.lag_curve_from_markers((), dur, sr, hop, azimuths=(l1,))
    ta = alone[:, 0]
    assert len(ta) == int(dur * sr / hop) and ta[-1] == dur     # no marker and no line at `duration`: lag 0 there
    out = (ta < 2.0) | (ta > 4.0)
    assert np.all(alone[out, 1] == 0.0) and np.array_equal(alone[~out, 1], f32(np.interp(ta, l1[0], l1[1]))[~out])
    # a line that covers `duration` moves the end of the grid
    l4 = (np.array([8.0, 11.0]), np.array([0.5, 0.5]), np.array([0.5, 0.5]), 100.0, 200.0)
    moved = pipeline.lag_curve_from_markers(marks, dur, sr, hop, azimuths=(l4,))
    assert abs(moved[-1, 0] - 10.5) < 1e-6 and len(moved) == int(moved[-1, 0] * sr / hop)


# ---- preconditions of the GPU cases (conditions on the inputs, proved with the oracles alone) -----------------------------------
def _check_row(a, b, ign, where):
    o = X.oracle_delay(a, b, ign)
    assert o.peak != len(a) - 1, where
    bd, bc = X.delay_bounds(o.fm, o.f0, o.fp, len(b))
    assert A.SAFETY * bd < 1e-6 and A.SAFETY * bc < 1e-6, (where, bd, bc)
    return o


@pytest.mark.parametrize("na,nb", A.BATCH_SHAPES)
def test_preconditions_batch_rows(na, nb):
    import scipy.signal
    a, b = A.batch_rows(na, nb, max(A.BATCH_WS))
    wa, wb = scipy.signal.get_window("hann", na), scipy.signal.get_window("hann", nb)
    for w in range(len(a)):
        for ign in (False, True):
            _check_row(a[w], b[w], ign, (na, nb, w, ign))
            _check_row(a[w] * wa, b[w] * wb, ign, (na, nb, w, ign, "hann"))


def test_preconditions_rival_and_status_rows():
    for name, (a, b, row, lags, loud) in A.rival_batches().items():
        same = X.same_direct(a[row], b[row]) if a.shape[1] * b.shape[1] <= (1 << 26) else X.same_fft(a[row], b[row])
        top, rivals = X.rivals_of(same)
        if name == "plateau":
            assert len(rivals) >= 64, (name, len(rivals))
        else:
            assert 1 <= len(rivals) <= 63, (name, len(rivals))
            o = _check_row(a[row], b[row], False, name)
            assert o.peak == lags[loud]
        for w in (0, 2):
            _check_row(a[w], b[w], False, (name, w))
            assert len(X.rivals_of(X.same_fft(a[w], b[w]))[1]) == 0
    a, b, edge, zero = A.status_batch()
    for w in range(len(a)):
        if w == edge:
            with pytest.raises(IndexError):
                X.oracle_delay(a[w], b[w])
        elif w == zero:
            assert not a[w].any() and not b[w].any()
        else:
            _check_row(a[w], b[w], False, ("status", w))


def test_preconditions_end_to_end_case():
    p = A.E2E
    ref2, src2, rc, sc = A.e2e_files()
    times, lags, wins = A.windows_of(ref2[:, rc], src2[:, sc], p["sr"], p["t0"], p["t1"], p["lag_curve"], p["dur"], p["overlap"])
    assert 35 <= len(times) <= 45
    shapes = {(len(a), len(b)) for a, b, _, _ in wins}
    assert len(shapes) >= 2, shapes
    assert any(ga[2] > 0 for _, _, ga, _ in wins) and any(ga[3] > 0 for _, _, ga, _ in wins)          # both file ends are crossed
    assert all(len(a) > 21 and len(b) > 21 for a, b, _, _ in wins)                                   # sosfiltfilt's padlen
    live = 0
    for i, (a, b, _, _) in enumerate(wins):
        o, fa, fb, flow = A.oracle_window(a, b, p["sr"], p["lower"], p["upper"])
        if o is None:
            continue
        live += 1
        assert o.peak != len(a) - 1, i
        bd, bc = X.delay_bounds(o.fm, o.f0, o.fp, len(b))
        assert A.SAFETY * bd < 1e-6 and A.SAFETY * bc < 1e-6, (i, bd, bc)
        assert A.SAFETY * bd < flow[0] < A.CEILING and A.SAFETY * bc < flow[1] < A.CEILING, (i, flow)      # with the filter's term
        assert abs(abs(o.corr) - A.REJECT) > 1e-6, (i, o.corr)
        assert len(X.rivals_of(X.same_direct(fa, fb))[1]) == 0, i
    assert live >= 30 and live < len(wins)                      # and some windows are silence (cut before the file's start)


def test_preconditions_golden_line(az_golden):
    """the fixture's 40 windows of rhythm.flac / rhythm+5percent.flac: the bound the GPU test holds azimuth_line to against the
    reference's own line (the float64 sums and the filter's pinned tolerance through the parabola, window by window) is finite, no
    oracle peak sits on the last lag, and the reference's own float64 line lies inside it.  This is programme material, not a built
    case: windows with |corr| of 0.1 .. 0.2 have a curvature of ~1e-4, so the bound ranges up to 1e-3 samples and has no common
    ceiling; the built end-to-end case above has (1e-6)."""
    from pyaudiorestoration_amd import io_ops
    g = az_golden
    gold = os.path.join(ROOT, "tests", "golden")
    ref_sig, sr, _ = io_ops.read_file(os.path.join(gold, "rhythm.flac"))
    src_sig, _, _ = io_ops.read_file(os.path.join(gold, "rhythm+5percent.flac"))
    rows = A.golden_window_bounds(g, ref_sig[:, 0], src_sig[:, 0])
    assert len(rows) == len(g["sample_times"]) == 40
    for i, (o, flow) in enumerate(rows):
        assert o is not None and o.peak != int(g["ref_geom"][i, 1:].sum()) - 1
        assert np.isfinite(flow[0]) and flow[0] < 2e-3 and flow[1] < 2e-5, (i, flow)
        assert abs((g["lags_raw"][i] - g["sample_lags"][i]) * sr - o.delay) <= flow[0] and abs(g["corrs"][i] - o.corr) <= flow[1], i


# ---- ABI without a GPU -------------------------------------------------------------------------------------------------------------
def test_abi_argument_errors_need_no_gpu():
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(8)
    fd = L.par_find_delay_batch_f64
    one = L.par_find_delay_batch_scratch_bytes(1000, 999, 1)

    def refused(rc, *words, code=1):
        assert rc == code, (rc, _lib.last_error())
        for w in words:
            assert w in _lib.last_error(), (w, _lib.last_error())
    refused(fd(0, None, 1000, 1000, p, 999, 999, 2, None, None, 0, p, one, p, p, p, None), "null")
    refused(fd(0, p, 1000, 1000, p, 999, 999, 2, None, None, 0, None, one, p, p, p, None), "null")
    refused(fd(0, p, 1000, 1000, p, 999, 999, 2, None, None, 0, p, one, p, p, None, None), "null")
    refused(fd(0, p, 1000, 2, p, 999, 999, 2, None, None, 0, p, one, p, p, p, None), "na 2")
    refused(fd(0, p, 1000, 1000, p, 999, 0, 2, None, None, 0, p, one, p, p, p, None), "nb 0")
    refused(fd(0, p, 1000, 1000, p, 999, 999, -1, None, None, 0, p, one, p, p, p, None), "n_win -1")
    refused(fd(0, p, 999, 1000, p, 999, 999, 2, None, None, 0, p, one, p, p, p, None), "pitch")
    refused(fd(0, p, 1000, 1000, p, 998, 999, 2, None, None, 0, p, one, p, p, p, None), "pitch")
    assert fd(0, p, 1000, 1000, p, 999, 999, 0, None, None, 0, p, one, p, p, p, None) == 0               # nothing to do
    refused(fd(0, p, 1 << 20, 1 << 20, p, 999, 2, 2, None, None, 0, p, one, p, p, p, None), "sectioned", code=3)
    refused(fd(0, p, 1000, 1000, p, 999, 999, 2, None, None, 0, p, one - 1, p, p, p, None), "less than one window", code=4)
    # scratch sizing: host arithmetic
    sb = L.par_find_delay_batch_scratch_bytes
    N = X.xc_fft_len(1000, 999)
    assert one >= 2 * N * 8 and sb(1000, 999, 0) == one
    sizes = [sb(1000, 999, w) for w in (1, 2, 3, 37, 1000, 10 ** 5, 10 ** 7)]
    assert sizes == sorted(sizes) and sizes[2] == 3 * one and sizes[-1] == sizes[-2]                      # monotone and capped
    assert sizes[-1] <= (1 << 30) + 32768 * (one - 2 * N * 8)
    big = sb(1 << 19, 1 << 19, 1000)
    assert big == 64 * sb(1 << 19, 1 << 19, 1) and big >= 1 << 30                                        # 1 GiB of transforms + tables
    assert sb(1 << 20, 2, 5) == 0                                                                        # not batched
    # gather: the geometry is checked on the host copy before anything is launched
    gw = L.par_gather_windows_f64

    def geom(*rows):
        return np.ascontiguousarray(np.array(rows, dtype=np.int64).T)
    ok = geom((0, 100, 5), (900, 100, 0))
    hp = lambda g: g.ctypes.data_as(ctypes.c_void_p)
    refused(gw(0, None, 2, 1000, p, p, p, hp(ok), 2, 110, p, 110, None), "null")
    refused(gw(0, p, 2, 1000, p, p, p, None, 2, 110, p, 110, None), "null")
    refused(gw(0, p, 2, 1000, p, p, p, hp(ok), 2, 110, p, 109, None), "pitch")
    for bad, word in ((geom((0, 100, 5), (901, 100, 0)), "window 1"), (geom((-1, 100, 5)), "window 0"), (geom((0, -1, 5)), "window 0"),
                      (geom((0, 100, 11)), "window 0"), (geom((0, 100, -1)), "window 0")):
        refused(gw(0, p, 2, 1000, p, p, p, hp(bad), bad.shape[1], 110, p, 110, None), word)
    assert gw(0, p, 2, 1000, p, p, p, hp(ok), 0, 110, p, 110, None) == 0
    assert "par_find_delay_batch_f64" in _lib.SIGNATURES and "par_gather_windows_f64" in _lib.SIGNATURES


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_azimuth_parses_and_refuses_without_a_gpu(tmp_path):
    import torch
    from pyaudiorestoration_amd import cli
    args = cli.parser().parse_args(["azimuth", "p.tapesync", "--ref", "a.flac", "--box", "1.5,300,2.0,3000", "--win", "0.05",
                                    "--overlap", "4", "--ignore-phase", "--out", "q.tapesync"])
    assert (args.cmd, args.project, args.ref, args.src, args.box) == ("azimuth", "p.tapesync", "a.flac", None, [1.5, 300.0, 2.0, 3000.0])
    assert (args.win, args.overlap, args.reject, args.ignore_phase, args.out) == (0.05, 4, 0.1, True, "q.tapesync")
    d = cli.parser().parse_args(["azimuth", "p.tapesync", "--ref", "a.flac", "--box", "1,2,3,4"])
    assert (d.win, d.overlap, d.reject, d.ignore_phase, d.out) == (0.2, 32, 0.1, False, None)
    with pytest.raises(SystemExit):
        cli.main(["azimuth", "p.tapesync", "--box", "1,2,3,4"])                   # --ref is required
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(SystemExit, match="no CPU fallback"):
        cli.main(["azimuth", str(tmp_path / "p.tapesync"), "--ref", str(tmp_path / "a.flac"), "--box", "1,2,3,4"])
