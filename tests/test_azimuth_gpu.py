"""The tape-sync azimuth mode on the GPU: par_find_delay_batch_f64 against the single call par_find_delay_f64 (bit for bit) and
the float64 oracles of tests/xcorr_inputs.py (4 x delay_bounds), par_gather_windows_f64 against Spectrum.get_signal restated,
pipeline.azimuth_line against the loop over pipeline.correlate_sources it replaces.  The preconditions of every input are proved
in tests/test_azimuth_cpu.py.  pytest -s prints the measured figures."""
import ctypes
import json
import os

import numpy as np
import pytest
import scipy.signal

import azimuth_inputs as A
import xcorr_inputs as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.25e11


@pytest.fixture(scope="module")
def C():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pyaudiorestoration_amd import correlation
    return correlation


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def pitched(rows, extra):
    """rows on the device at a pitch larger than their length, NaN in the gap -> (the (W, n) view, the whole buffer)"""
    import torch
    W, n = rows.shape
    buf = torch.full((W, n + extra), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :n] = torch.from_numpy(rows).cuda()
    return buf[:, :n], buf


def run_batch(a, b, ign, window_name, scratch_bytes=None):
    """the ABI call itself on pitched rows, outputs between sentinel cells -> (delay, corr, status, rows of a and b afterwards)"""
    import torch
    from pyaudiorestoration_amd import _dev, _lib
    L = _lib.lib()
    W, na = a.shape
    nb = b.shape[1]
    a_v, a_buf = pitched(a, 5)
    b_v, b_buf = pitched(b, 3)
    out = torch.full((3, W + 2), SENTINEL, dtype=torch.float64, device="cuda")
    st = torch.full((W + 2,), -77, dtype=torch.int32, device="cuda")
    nbytes = int(L.par_find_delay_batch_scratch_bytes(na, nb, W)) if scratch_bytes is None else int(scratch_bytes)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    wa = wb = None
    if window_name:
        wa = torch.from_numpy(scipy.signal.get_window(window_name, na)).cuda()
        wb = torch.from_numpy(scipy.signal.get_window(window_name, nb)).cuda()
    _lib.check(L.par_find_delay_batch_f64(0, _dev.ptr(a_v), a_buf.stride(0), na, _dev.ptr(b_v), b_buf.stride(0), nb, W,
                                          _dev.ptr(wa) if window_name else None, _dev.ptr(wb) if window_name else None, int(ign),
                                          _dev.ptr(scratch), nbytes, _dev.ptr(out[0, 1:]), _dev.ptr(out[1, 1:]), _dev.ptr(st[1:]),
                                          _dev.stream_ptr(0)))
    torch.cuda.synchronize()
    o, s = out.cpu().numpy(), st.cpu().numpy()
    assert np.all(o[:2, 0] == SENTINEL) and np.all(o[:2, -1] == SENTINEL) and np.all(o[2] == SENTINEL) and s[0] == s[-1] == -77
    ab, bb = a_buf.cpu().numpy(), b_buf.cpu().numpy()
    assert np.all(np.isnan(ab[:, na:])) and np.all(np.isnan(bb[:, nb:]))               # the gaps between the rows are untouched
    return o[0, 1:-1], o[1, 1:-1], s[1:-1], ab[:, :na], bb[:, :nb]


def single(C, a, b, ign, window_name):
    """correlation.find_delay row by row (on copies)"""
    d, c = np.empty(len(a)), np.empty(len(a))
    for w in range(len(a)):
        d[w], c[w] = C.find_delay(a[w].copy(), b[w].copy(), ignore_phase=ign, window_name=window_name)
    return d, c


# ---- 1. batch against the single call ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window_name", [None, "hann"])
@pytest.mark.parametrize("ign", [False, True])
@pytest.mark.parametrize("na,nb", A.BATCH_SHAPES)
def test_batch_equals_single_call(C, na, nb, ign, window_name):
    """W = 1, 2, 37 rows of white, narrow-band and tone takes: find_delay_batch equals find_delay row by row, bit for bit.  The single
    call is the batch of one row through the same kernels, so the equality says that a row's result does not depend on its
    neighbours, its pitch, W or the entry point; the accuracy statement is the pin of every row to the fsum oracle within
    4 x delay_bounds.  Pitched rows, sentinels around the outputs, a second run identical"""
    a, b = A.batch_rows(na, nb, max(A.BATCH_WS))
    want_d, want_c = single(C, a, b, ign, window_name)
    wa = scipy.signal.get_window(window_name, na) if window_name else 1.0
    wb = scipy.signal.get_window(window_name, nb) if window_name else 1.0
    worst = (0.0, 0.0)
    for w in range(len(a)):
        o = X.oracle_delay(a[w] * wa, b[w] * wb, ign)
        bd, bc = X.delay_bounds(o.fm, o.f0, o.fp, nb)
        r = (abs(want_d[w] - o.delay) / bd, abs(want_c[w] - o.corr) / bc)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
        assert max(r) <= A.SAFETY, (na, nb, w, ign, window_name, want_d[w], want_c[w], o, r)
    print(f"\n{na} x {nb} ign {ign} window {window_name}: worst delay error {worst[0]:.2e}, corr error {worst[1]:.2e} of the derived bounds",
          end="")
    for W in A.BATCH_WS:
        aw, bw = a[:W].copy(), b[:W].copy()
        d, c = C.find_delay_batch(aw, bw, ignore_phase=ign, window_name=window_name)
        assert d.dtype == c.dtype == np.float64 and d.shape == c.shape == (W,)
        assert same_bits(d, want_d[:W]) and same_bits(c, want_c[:W]), (W, np.flatnonzero(bits(d) != bits(want_d[:W])), d, want_d[:W])
        if window_name:                                                   # windowed in place, like find_delay
            assert same_bits(aw, a[:W] * wa) and same_bits(bw, b[:W] * wb)
        else:
            assert same_bits(aw, a[:W]) and same_bits(bw, b[:W])
        d1, c1, s1, _, _ = run_batch(a[:W], b[:W], ign, window_name)
        d2, c2, s2, _, _ = run_batch(a[:W], b[:W], ign, window_name)
        assert same_bits(d1, want_d[:W]) and same_bits(c1, want_c[:W]) and not s1.any()
        assert same_bits(d1, d2) and same_bits(c1, c2) and np.array_equal(s1, s2)


# ---- 2. chunking -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("na,nb", [(1000, 999), (4097, 4097)])
def test_results_do_not_depend_on_the_scratch_size(C, na, nb):
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    a, b = A.batch_rows(na, nb, 37, seed=1)
    one = int(L.par_find_delay_batch_scratch_bytes(na, nb, 1))
    asked = int(L.par_find_delay_batch_scratch_bytes(na, nb, 37))
    assert asked == 37 * one
    runs = [run_batch(a, b, True, "hann", nbytes) for nbytes in (one, 3 * one, 3 * one + one // 2, asked)]
    for d, c, s, ra, rb in runs[1:]:
        assert same_bits(d, runs[0][0]) and same_bits(c, runs[0][1]) and np.array_equal(s, runs[0][2])
        assert same_bits(ra, runs[0][3]) and same_bits(rb, runs[0][4])
    assert np.all(np.isfinite(runs[0][0])) and not runs[0][2].any()
    with pytest.raises(_lib.ParError, match="less than one window"):
        run_batch(a, b, True, "hann", one - 1)


# ---- 3. rivals inside a batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["K2", "K32", "plateau"])
def test_rivals_inside_a_batch(C, name):
    """a rival_case row (a plateau row) between two ordinary rows: every row is decided like its single call"""
    a, b, row, lags, loud = A.rival_batches()[name]
    want_d, want_c = single(C, a, b, False, None)
    d, c = C.find_delay_batch(a.copy(), b.copy())
    assert same_bits(d, want_d) and same_bits(c, want_c), (d, want_d)
    n = a.shape[1]
    if name == "plateau":
        assert np.min(np.abs(d[row] + n // 2 - lags)) <= 0.5                        # ON one of the copies (the stated limit)
    else:
        assert round(d[row] + n // 2) == lags[loud]                                  # the exact values name the louder copy
        o = X.oracle_delay(a[row], b[row])
        bd, bc = X.delay_bounds(o.fm, o.f0, o.fp, n)
        assert abs(d[row] - o.delay) <= A.SAFETY * bd and abs(c[row] - o.corr) <= A.SAFETY * bc
    # the special row alone, and with its neighbours swapped: the same bits
    d1, c1 = C.find_delay_batch(a[row:row + 1].copy(), b[row:row + 1].copy())
    d3, c3 = C.find_delay_batch(a[::-1].copy(), b[::-1].copy())
    assert same_bits(d1, d[row:row + 1]) and same_bits(c1, c[row:row + 1]) and same_bits(d3, d[::-1]) and same_bits(c3, c[::-1])


# ---- 4. row status -----------------------------------------------------------------------------------------------------------------
def test_row_status_and_silence(C):
    import torch
    a, b, edge, zero = A.status_batch()
    d, c, s, _, _ = run_batch(a, b, False, None)
    assert s.tolist() == [0, 1, 0, 0, 0]
    assert np.isnan(d[edge]) and np.isnan(c[edge]) and np.isnan(d[zero]) and np.isnan(c[zero])
    keep = [w for w in range(len(a)) if w not in (edge, zero)]
    want_d, want_c = single(C, a[keep], b[keep], False, None)
    assert same_bits(d[keep], want_d) and same_bits(c[keep], want_c)
    with pytest.raises(IndexError, match=r"index 1000 is out of bounds for axis 0 with size 1000 \(row 1\)"):
        C.find_delay_batch(a.copy(), b.copy())
    with pytest.raises(IndexError):
        C.find_delay(a[edge].copy(), b[edge].copy())
    # silence raises nothing, in the batch and alone, and leaves no HIP error behind
    rest = [w for w in range(len(a)) if w != edge]
    d2, c2 = C.find_delay_batch(a[rest].copy(), b[rest].copy(), window_name="hann")
    assert np.isnan(d2[2]) and np.isnan(c2[2]) and np.all(np.isfinite(np.delete(d2, 2)))
    ds, cs = C.find_delay(a[zero].copy(), b[zero].copy())
    assert np.isnan(ds) and np.isnan(cs)
    from pyaudiorestoration_amd import _dev, _lib
    assert _lib.lib().par_stream_sync(0, _dev.stream_ptr(0)) == 0, _lib.last_error()      # hipStreamSynchronize reports a fault of the queue
    torch.cuda.synchronize()
    assert torch.zeros(4, device="cuda").sum().item() == 0.0                               # and the device still takes work
    dt, ct, stt = C.find_delay_batch_dev(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert stt.cpu().tolist() == [0, 1, 0, 0, 0] and same_bits(dt.cpu().numpy(), d) and same_bits(ct.cpu().numpy(), c)
    e, f = C.find_delay_batch(np.zeros((0, 100)), np.zeros((0, 90)))
    assert e.shape == f.shape == (0,)


# ---- 5. in-place window ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("na,nb", [(1000, 64), (4097, 4096)])
def test_window_is_applied_in_place(C, na, nb):
    a, b = A.batch_rows(na, nb, 7, seed=2)
    _, _, _, ra, rb = run_batch(a, b, False, "hann")
    assert same_bits(ra, a * scipy.signal.get_window("hann", na)) and same_bits(rb, b * scipy.signal.get_window("hann", nb))
    _, _, _, ra, rb = run_batch(a, b, False, None)
    assert same_bits(ra, a) and same_bits(rb, b)


# ---- 6. gather ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [g for g in A.geometry_cases() if not g.name.startswith("empty")], ids=lambda g: g.name)
def test_gather_equals_get_signal(g):
    """channel 1 of an interleaved 2-channel float32 file between sentinel cells: every row equals Spectrum.get_signal's window,
    zero up to n_out, untouched behind it"""
    import torch
    from pyaudiorestoration_amd import _dev, _lib, pipeline
    ref, src = A.geometry_signals(g)
    _, _, ref_geom, src_geom = pipeline.azimuth_windows(g.len_ref, g.len_src, g.sr, g.t0, g.t1, g.lag_curve, g.dur, g.overlap)
    _, _, want = A.windows_of(ref, src, g.sr, g.t0, g.t1, g.lag_curve, g.dur, g.overlap)
    for sig, geom, k in ((ref, ref_geom, 0), (src, src_geom, 1)):
        n, W = len(sig), len(geom)
        file2 = np.full((n + 2, 2), 3.0e33, dtype=np.float32)                          # poison: channel 0 and a cell at either end
        file2[1:-1, 1] = sig
        file_t = torch.from_numpy(file2).cuda().reshape(-1)
        n_out = int(np.max(geom[:, 1:].sum(axis=1))) + 3
        pitch = n_out + 5
        out = torch.full((W + 2, pitch), SENTINEL, dtype=torch.float64, device="cuda")
        host = np.ascontiguousarray(geom[:, :3].T)
        geo_t = torch.from_numpy(host).cuda()
        _lib.check(_lib.lib().par_gather_windows_f64(0, _dev.ptr(file_t[3:]), 2, n, _dev.ptr(geo_t[0]), _dev.ptr(geo_t[1]), _dev.ptr(geo_t[2]),
                                                     host.ctypes.data_as(ctypes.c_void_p), W, n_out, _dev.ptr(out[1]), pitch,
                                                     _dev.stream_ptr(0)))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[0] == SENTINEL) and np.all(got[-1] == SENTINEL) and np.all(got[1:-1, n_out:] == SENTINEL)
        for w in range(W):
            cut = want[w][k]
            assert np.array_equal(got[1 + w, :len(cut)], cut.astype(np.float64)) and not got[1 + w, len(cut):n_out].any(), (g.name, k, w)
        # the Python wrapper: rows of exactly their length
        rows = [r for r in range(W) if geom[r, 1:].sum() == geom[0, 1:].sum()]
        t = pipeline.gather_windows_dev(file_t[2:], 2, n, 1, geom[rows], int(geom[0, 1:].sum()), 0)
        assert np.array_equal(t.cpu().numpy(), np.stack([want[r][k] for r in rows]).astype(np.float64))
    bad = geom.copy()
    bad[-1, 0] = n - bad[-1, 1] + 1                                                    # one sample past the end: refused, nothing written
    with pytest.raises(_lib.ParError, match=f"window {W - 1}"):
        pipeline.gather_windows_dev(file_t[2:], 2, n, 1, bad, n_out, 0)


# ---- 7. azimuth_line end to end ----------------------------------------------------------------------------------------------------
def test_azimuth_line_end_to_end(C, monkeypatch):
    """the batch against the loop over pipeline.correlate_sources(..., window_name="hann") it replaces, bit for bit; both against the
    per-window float64 oracle within azimuth_inputs.flow_bounds (the float64 sums at 4 x and K_sosfiltfilt's pinned 1e-9 through the
    parabola), which test_azimuth_cpu.py proves to be below 1e-6 samples / 1e-6 for every window of this case"""
    import torch
    from pyaudiorestoration_amd import pipeline
    p = A.E2E
    sr = p["sr"]
    ref2, src2, rc, sc = A.e2e_files()
    times, lags, wins = A.windows_of(ref2[:, rc], src2[:, sc], sr, p["t0"], p["t1"], p["lag_curve"], p["dur"], p["overlap"])
    assert len({(len(a), len(b)) for a, b, _, _ in wins}) >= 2
    loop_raw, loop_c = np.empty(len(times)), np.empty(len(times))
    for i, (a, b, _, _) in enumerate(wins):
        time_delay, loop_c[i] = pipeline.correlate_sources(a, b, sr, p["lower"], p["upper"], False, "hann")
        loop_raw[i] = lags[i] + time_delay
    line = pipeline.azimuth_line(ref2, src2, sr, p["t0"], p["t1"], p["lower"], p["upper"], p["lag_curve"], p["dur"], p["overlap"], A.REJECT,
                                 ref_channel=rc, src_channel=sc)
    assert isinstance(line, pipeline.AzimuthLine) and np.array_equal(line.times, times) and (line.lower, line.upper) == (p["lower"], p["upper"])
    assert same_bits(line.lags_raw, loop_raw) and same_bits(line.corrs, loop_c), (line.lags_raw - loop_raw, line.corrs - loop_c)
    silent = worst_d = worst_c = 0
    for i, (a, b, _, _) in enumerate(wins):
        o, _, _, flow = A.oracle_window(a, b, sr, p["lower"], p["upper"])
        if o is None:
            silent += 1
            assert np.isnan(line.lags_raw[i]) and np.isnan(line.corrs[i])
            continue
        ed, ec = abs((line.lags_raw[i] - lags[i]) * sr - o.delay), abs(line.corrs[i] - o.corr)
        worst_d, worst_c = max(worst_d, ed), max(worst_c, ec)
        assert flow[0] < A.CEILING and flow[1] < A.CEILING and ed <= flow[0] and ec <= flow[1], (i, ed, ec, flow)
    print(f"\nazimuth_line: {len(times)} windows ({silent} silent), worst |delay - oracle| {worst_d:.2e} samples, |corr - oracle| {worst_c:.2e}",
          end="")
    assert silent >= 1 and np.array_equal(line.lags, pipeline.azimuth_reject(line.lags_raw, line.corrs, p["overlap"], A.REJECT))
    assert np.all(np.isfinite(line.lags))
    # small chunks, device tensors in, and the other phase setting: the same line / still the loop's bits
    small = pipeline.azimuth_line(torch.from_numpy(ref2).cuda(), torch.from_numpy(src2).cuda(), sr, p["t0"], p["t1"], p["lower"], p["upper"],
                                  p["lag_curve"], p["dur"], p["overlap"], A.REJECT, ref_channel=rc, src_channel=sc, max_bytes=1 << 19)
    assert same_bits(small.lags_raw, line.lags_raw) and same_bits(small.corrs, line.corrs)
    # a shape the batch refuses (the sectioned form: windows of more than 2^20 lags) runs window by window: the same bits
    from pyaudiorestoration_amd import _lib

    def refuse(na, nb, n_win):
        raise _lib.ParUnsupported(3, "refused for the test")
    monkeypatch.setattr(C, "batch_scratch_bytes", refuse)
    slow = pipeline.azimuth_line(ref2, src2, sr, p["t0"], p["t1"], p["lower"], p["upper"], p["lag_curve"], p["dur"], p["overlap"], A.REJECT,
                                 ref_channel=rc, src_channel=sc)
    monkeypatch.undo()
    assert same_bits(slow.lags_raw, line.lags_raw) and same_bits(slow.corrs, line.corrs) and same_bits(slow.lags, line.lags)
    cfg = line.to_cfg()
    assert len(cfg) == 5 and cfg[0] == list(times) and isinstance(cfg[1], list) and cfg[3:] == (p["lower"], p["upper"])
    json.dumps(cfg)
    empty = pipeline.azimuth_line(ref2, src2, sr, 0.3, 0.3, p["lower"], p["upper"], p["lag_curve"], p["dur"], p["overlap"])
    assert len(empty.times) == len(empty.lags) == len(empty.corrs) == 0


def test_lag_curve_with_the_golden_line_filtered(C):
    """LagLine.update with a 0 .. 2 Hz band over the two markers of rhythm.tapesync and the line the reference measured: the grid bit
    for bit, the filtered curve within 1e-9 of the reference's (scipy's sosfiltfilt there, K_sosfiltfilt here)"""
    from pyaudiorestoration_amd import pipeline
    g = np.load(os.path.join(ROOT, "tests", "golden", "azimuth.npz"))
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "rhythm.tapesync")))
    line = (g["sample_times"], g["lags"], g["corrs"], float(g["lower"]), float(g["upper"]))
    curve = pipeline.lag_curve_from_markers(cfg["markers"], float(g["duration"]), int(g["sr"]), int(g["hop"]), int(g["smoothing"]),
                                            bands=tuple(g["bands"]), azimuths=(line,))
    assert curve.shape == (int(g["curve_len"]), 2)
    got, want = curve[g["curve_rows"]], g["curve_filtered"]
    err = float(np.max(np.abs(got[:, 1] - want[:, 1])))
    print(f"\nfiltered lag curve: max |curve - reference| {err:.2e} s", end="")
    assert np.array_equal(got[:, 0].astype(want.dtype), want[:, 0]) and err <= 1e-9


def test_golden_line_and_cli(C, tmp_path):
    """rhythm.flac / rhythm+5percent.flac with the fixture's selection and the lag curve the reference sampled: the line the reference
    measured, window by window within azimuth_inputs.flow_bounds.  `cli azimuth` measures against the project's own curve and appends the line."""
    from pyaudiorestoration_amd import cli, io_ops, pipeline
    g = np.load(os.path.join(ROOT, "tests", "golden", "azimuth.npz"))
    gold = os.path.join(ROOT, "tests", "golden")
    sr = int(g["sr"])
    ref_sig, _, _ = io_ops.read_file(os.path.join(gold, "rhythm.flac"))
    src_sig, _, _ = io_ops.read_file(os.path.join(gold, "rhythm+5percent.flac"))
    args = (float(g["t0"]), float(g["t1"]), float(g["lower"]), float(g["upper"]))
    kw = dict(dur=float(g["dur"]), overlap=int(g["overlap"]), reject=float(g["reject"]))
    line = pipeline.azimuth_line(ref_sig, src_sig, sr, *args, g["lag_curve0"], **kw)
    assert np.array_equal(line.times, g["sample_times"])
    # window by window inside flow_bounds of the fsum oracle, as the reference's own line is (test_azimuth_cpu.py); so the two lines
    # are within twice that of each other
    ed = np.abs(line.lags_raw - g["lags_raw"]) * sr
    ec = np.abs(line.corrs - g["corrs"])
    bounds = A.golden_window_bounds(g, ref_sig[:, 0], src_sig[:, 0])
    bd, bc = np.array([f[0] for _, f in bounds]), np.array([f[1] for _, f in bounds])
    od = np.abs((line.lags_raw - g["sample_lags"]) * sr - np.array([o.delay for o, _ in bounds]))
    oc = np.abs(line.corrs - np.array([o.corr for o, _ in bounds]))
    print(f"\nazimuth_line against the reference's line: raw lags {ed.max():.2e} samples, corrs {ec.max():.2e}; against the fsum oracle "
          f"{od.max():.2e} samples, {oc.max():.2e}; bounds {bd.min():.1e} .. {bd.max():.1e} samples, {bc.min():.1e} .. {bc.max():.1e}", end="")
    assert np.all(od <= bd) and np.all(oc <= bc) and np.all(ed <= 2 * bd) and np.all(ec <= 2 * bc)
    assert np.max(np.abs(line.lags - g["lags"])) * sr <= 2 * bd.max()                # the median picks one of the raw values
    out = tmp_path / "rhythm2.tapesync"
    project = os.path.join(gold, "rhythm.tapesync")
    box = f"{args[0]},{args[2]},{args[1]},{args[3]}"
    rc = cli.main(["azimuth", project, "--ref", os.path.join(gold, "rhythm.flac"), "--src", os.path.join(gold, "rhythm+5percent.flac"),
                   "--box", box, "--win", str(kw["dur"]), "--overlap", str(kw["overlap"]), "--reject", str(kw["reject"]), "--out", str(out)])
    assert rc == 0
    new = json.load(open(out))
    old = json.load(open(project))
    assert "markers" not in new and new["lags"] == old["markers"] and len(new["azimuths"]) == 1
    curve0 = pipeline.project_lag_curve(old, len(src_sig) / sr, sr)
    mine = pipeline.azimuth_line(ref_sig, src_sig, sr, *args, curve0, **kw)
    times, lags, corrs, lower, upper = new["azimuths"][0]
    assert np.array_equal(times, mine.times) and same_bits(lags, mine.lags) and same_bits(corrs, mine.corrs) and (lower, upper) == args[2:]
    curve = pipeline.project_lag_curve(new, float(g["duration"]), sr)
    assert curve.shape == (int(g["curve_len"]), 2)
    cli.main(["azimuth", project, "--ref", os.path.join(gold, "rhythm.flac"), "--src", os.path.join(gold, "rhythm+5percent.flac"), "--box", box,
              "--win", str(kw["dur"]), "--overlap", str(kw["overlap"])])                  # no --out: nothing is written
    assert sorted(os.listdir(tmp_path)) == ["rhythm2.tapesync"]
