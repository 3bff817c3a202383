"""The stereo balance tool without a GPU: the host restatements of pypan.py against what the reference computed
(tests/golden/pypan.npz, tools/gen_golden_pypan.py), the statements and bounds of tests/pan_np.py on the fixture alone, the C
ABI's argument checks, and the CLI's refusal."""
import ctypes
import math
import os

import numpy as np
import pytest

import pan_np as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g(golden):
    return golden["pypan"]


@pytest.fixture(scope="module")
def tape():
    return N.stereo_tape()


def _geometry(g, zeropad=1):
    sr, fft, hop, n = int(g["sr"]), int(g["fft_size"]), int(g["hop"]), int(g["n"])
    return sr, fft, hop, fft * zeropad // 2 + 1, (n + 2 * (fft // 2) - fft) // hop + 1


def test_fixture_input_is_the_seeded_tape(g, tape):
    assert int(g["seed"]) == N.SEED and int(g["n"]) == len(tape) == N.N and int(g["sr"]) == N.SR
    assert int(g["fft_size"]) == N.FFT_SIZE and int(g["fft_overlap"]) == N.FFT_OVERLAP
    assert float(np.abs(tape[:, 0] - tape[:, 1]).max()) > 0.1           # two different channels


def test_box_to_cells_equals_the_references_integers(g):
    from pyaudiorestoration_amd import pypan
    for zp, boxes, cells in ((1, g["boxes"], g["cells"]), (int(g["zeropad2"]), g["boxes_zp2"], g["cells_zp2"])):
        sr, fft, hop, bins, frames = _geometry(g, zp)
        for (a0, a1, b0, b1), want in zip(boxes, cells):
            assert pypan.box_to_cells((a0, a1), (b0, b1), sr, fft, hop, bins, frames) == tuple(int(v) for v in want)
    kinds = [tuple(c) for c in g["cells"]]
    assert any(c[2] == 0 for c in kinds) and any(c[3] == _geometry(g)[4] for c in kinds) and any(c[0] == c[1] == 1 for c in kinds)
    assert any(c[2] == c[3] for c in kinds)                               # a box that collapsed


def test_box_to_cells_hand_cases():
    from pyaudiorestoration_amd.pypan import box_to_cells
    sr, fft, hop, bins, frames = 44100, 4096, 512, 2049, 1000
    cell = lambda a, b: box_to_cells(a, b, sr, fft, hop, bins, frames)
    # a start time of exactly 0 is falsy: the first frame stays 0 -- and so does an END time of 0 leave the last frame alone
    assert cell((0.0, 100), (2.0, 200))[2:] == (0, int(2.0 * sr / hop))
    assert cell((0.0, 100), (0.0, 200))[2:] == (0, frames)
    assert cell((-1.0, 100), (0.0, 200))[2:] == (0, frames)               # sorted: t0 = -1 (max with 0), t1 = 0 (falsy)
    # an end beyond the file stops at the frame count
    assert cell((1.0, 100), (99.0, 200))[2:] == (int(1.0 * sr / hop), frames)
    # frequencies below 1 Hz and above sr // 2 - 1
    assert cell((1, 0.0), (2, 1e9))[:2] == (1, min(bins - 3, int(round((sr // 2 - 1) * fft / sr))))
    assert cell((1, -5.0), (2, 0.5))[:2] == (1, 1)
    # Python's round: ties to even.  f * fft / sr == k + 0.5 exactly for sr = fft = 4096 (f itself)
    tie = lambda f: box_to_cells((1, f), (2, f), 4096, 4096, 512, 2049, 100)[0]
    assert tie(10.5) == 10 and tie(11.5) == 12 and tie(12.5) == 12 and round(10.5) == 10
    # clamps to 1 and num_bins - 3
    assert box_to_cells((1, 1), (2, 2047), 4096, 4096, 512, 2049, 100)[:2] == (1, 2046)
    assert box_to_cells((1, 2040), (2, 2046), 4096, 4096, 512, 2049, 100)[:2] == (2040, 2046)
    # fft_size enters without the zero-padding factor: the bins of a padded spectrum are still counted in unpadded steps
    assert box_to_cells((1, 1000), (2, 1500), 4096, 4096, 512, 2 * 2048 + 1, 100)[:2] == (1000, 1500)
    # a box narrower than a frame or a bin collapses to empty
    c = cell((1.0, 1000.0), (1.001, 1000.2))
    assert c[0] == c[1] and c[2] == c[3]


def test_pan_line_equals_the_references(g):
    from pyaudiorestoration_amd import pypan
    sr, hop, dur = int(g["sr"]), int(g["hop"]), float(g["duration"])
    rows = [tuple(r) for r in g["markers"]]
    assert [pypan.PanSample.from_cfg(*r).t for r in rows] != sorted(pypan.PanSample.from_cfg(*r).t for r in rows)   # pushed unsorted
    want = g["pan_data"]
    got = pypan.pan_line(rows, dur, sr, hop)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(pypan.pan_line([pypan.PanSample.from_cfg(*r) for r in reversed(rows)], dur, sr, hop), want)
    one = pypan.pan_line(rows[:1], dur, sr, hop)
    assert one.shape == want.shape and np.all(one[:, 1] == rows[0][4]) and np.array_equal(one[:, 0], want[:, 0])
    empty = pypan.pan_line([], dur, sr, hop)
    assert empty.dtype == np.float32 and empty.tolist() == [[0.0, 0.0], [999.0, 0.0]]        # BaseLine.empty
    s = pypan.PanSample((1.0, 20.0), (3.0, 40.0), 1.25)
    assert s.t == 2.0 and s.to_cfg() == (1.0, 20.0, 3.0, 40.0, 1.25)


def test_numpy_statement_of_apply_equals_the_fixture_rows(g, tape):
    idx, sr = g["af_idx"].astype(np.int64), int(g["sr"])
    xp, fp = g["pan_data"][:, 0] * sr, g["pan_data"][:, 1]
    af = np.interp(np.arange(len(tape)), xp, fp)
    assert np.array_equal(af[idx], g["af"])
    assert str(g["out_dtype"]) == "float64"                       # float32 x float64; the FLOAT file stores its float32 rounding
    assert np.array_equal((tape[:, 1] * af)[idx], g["out"])
    assert np.array_equal(N.interp_apply(tape[:, 1], xp, fp)[idx], g["out"].astype(np.float32))
    knots = np.round(np.array([(r[0] + r[2]) / 2 for r in g["markers"]]) * sr).astype(np.int64)
    assert all(k in idx for k in knots if k < len(tape)) and np.sum(knots < len(tape)) >= 4      # one marker lies behind the file's end


def test_reference_alone_is_inside_the_summation_term(g):
    """the fixture's fac of the small box against math.fsum of the fixture's own cells: the reference's summation error, which is
    what B_ref's summation term is scaled from"""
    k = int(g["small_box"])
    q = g["small_L"] / g["small_R"]
    exact, cnt, _ = N.fsum_mean(q)
    bl, bu, f0, f1 = g["cells"][k]
    assert cnt == (bu - bl) * (f1 - f0) == q.size
    s0 = abs(float(g["fac"][k]) - exact) / abs(exact)
    assert s0 == float(g["s0"]) == N.S0_MEASURED
    assert abs(float(g["fac"][k]) - exact) <= N.summation_term(exact, cnt, s0, cnt)
    assert str(g["spectra_dtype"]) in ("float32", "float64")


def test_b_ref_is_in_its_linear_range_and_small(g, tape):
    sr, fft, hop, _, _ = _geometry(g)
    for cell, fac in zip(g["cells"], g["fac"]):
        if math.isnan(fac):
            continue
        term, worst = N.transform_term(tape, 0, 1, fft, hop, 1, cell)
        assert worst < 0.25 and 0 < term < 2e-4 * fac
        # the float64 statement of the measurement agrees with the reference far inside the bound
        bl, bu, f0, f1 = cell
        fr = np.arange(f0, f1)
        m = np.mean(N.mags64(tape[:, 0], fft, hop, 1, fr)[:, bl:bu] / N.mags64(tape[:, 1], fft, hop, 1, fr)[:, bl:bu])
        assert abs(m - fac) <= 0.01 * N.b_ref(tape, 0, 1, fft, hop, 1, cell, fac, float(g["s0"]), 95)


def test_fsum_statement():
    q = np.array([[1.0, np.nan], [np.inf, 2.0]], dtype=np.float32)
    assert N.fsum_mean(q) == (math.inf, 3, math.inf)
    assert N.fsum_mean(np.array([np.nan]))[1] == 0 and math.isnan(N.fsum_mean(np.array([np.nan]))[0])
    assert N.fsum_mean(np.array([1e16, 1.0, -1e16]))[0] == 1.0 / 3
    assert N.b_ratio(1000, 2.0) == 2000 * 2.0 ** -52


def test_abi_argument_errors_without_a_gpu():
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(16)
    box = lambda *v: np.array(v, dtype=np.int32).reshape(-1, 4)
    ok = box(1, 5, 0, 10)
    need = L.par_pan_ratio_scratch_bytes(ok.ctypes.data, 1)
    assert need == 16 + 10 * 16 == L.par_stft_pan_scratch_bytes(ok.ctypes.data, 1)
    assert L.par_pan_ratio_scratch_bytes(box(1, 5, 0, 10, 5, 5, 0, 10, 1, 5, 7, 7, 2, 9, 3, 4).ctypes.data, 4) == 48 + 11 * 16
    assert L.par_pan_ratio_scratch_bytes(None, 1) == 0 and L.par_pan_ratio_scratch_bytes(ok.ctypes.data, 0) == 0
    # entry 1: nulls, sizes, a box outside the spectrogram, scratch
    ratio = lambda magL=p, magR=p, frames=10, bins=9, pitch=0, boxes=p, host=ok, n_box=1, fac=p, cnt=p, scr=p, nbytes=need: \
        L.par_pan_ratio_f32(0, magL, magR, frames, bins, pitch, boxes, host.ctypes.data if host is not None else None, n_box, fac, cnt,
                            scr, nbytes, None)
    for kw in ({"magL": None}, {"magR": None}, {"boxes": None}, {"host": None}, {"fac": None}, {"cnt": None}, {"scr": None}):
        assert ratio(**kw) == 1 and "null" in _lib.last_error(), kw
    for kw in ({"frames": 0}, {"bins": 0}, {"pitch": 8}, {"n_box": 0}, {"scr": ctypes.c_void_p(24)}):
        assert ratio(**kw) == 1, kw
    for bad in (box(1, 10, 0, 10), box(-1, 5, 0, 10), box(1, 5, 0, 11), box(1, 5, -1, 10), box(1, 5, 11, 11)):
        assert ratio(host=bad) == 1 and "leaves the spectrogram" in _lib.last_error(), bad
    assert ratio(nbytes=need - 1) == 4 and "scratch" in _lib.last_error()                  # PAR_ERR_WORKSPACE
    # entry 2: nulls, sizes, unsupported transform sizes, boxes against ITS frame and bin counts, scratch
    fused = lambda xL=p, xR=p, stride=2, n=4096, n_fft=1024, hop=256, zp=1, win=p, boxes=p, host=ok, n_box=1, fac=p, cnt=p, scr=p, \
        nbytes=need: L.par_stft_pan_ratio_f32(0, xL, xR, stride, n, n_fft, hop, zp, win, boxes,
                                              host.ctypes.data if host is not None else None, n_box, fac, cnt, scr, nbytes, None)
    for kw in ({"xL": None}, {"xR": None}, {"win": None}, {"boxes": None}, {"host": None}, {"fac": None}, {"cnt": None}, {"scr": None}):
        assert fused(**kw) == 1 and "null" in _lib.last_error(), kw
    for kw in ({"stride": 0}, {"n": 0}, {"hop": 0}, {"zp": 0}, {"n_box": 0}):
        assert fused(**kw) == 1, kw
    for kw in ({"n_fft": 1000}, {"n_fft": 8}, {"n_fft": 16384, "zp": 2}, {"n_fft": 32768}):
        assert fused(**kw) == 3 and "power of two" in _lib.last_error(), kw
    with pytest.raises(_lib.ParUnsupported):
        _lib.check(fused(n_fft=32768))
    assert L.par_stft_frames(4096, 1024, 256) == 17
    # (every call here stops before a device call: the pointers are not memory)
    assert fused(host=box(1, 514, 0, 17), nbytes=1 << 20) == 1 and "leaves the spectrogram" in _lib.last_error()
    assert fused(host=box(1, 513, 0, 18), nbytes=1 << 20) == 1 and "leaves the spectrogram" in _lib.last_error()
    assert fused(nbytes=need - 1) == 4 and "scratch" in _lib.last_error()
    # entry 3
    app = lambda sig=p, ss=1, n=10, xp=p, fp=p, m=2, out=p, os_=1: L.par_pan_apply_f32(0, sig, ss, n, xp, fp, m, out, os_, None)
    for kw in ({"sig": None}, {"xp": None}, {"fp": None}, {"out": None}):
        assert app(**kw) == 1 and "null" in _lib.last_error(), kw
    assert app(m=0) == 1 and "np.interp raises" in _lib.last_error()
    for kw in ({"n": -1}, {"ss": 0}, {"os_": 0}):
        assert app(**kw) == 1, kw
    assert app(n=0) == 0                                                                   # nothing to do, before any device call


def test_cli_pan_refuses_without_a_gpu(tmp_path):
    import torch
    from pyaudiorestoration_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["pan"])                                                                  # FILE is required
    args = cli.parser().parse_args(["pan", "--box", "1,2,3,4", "--box", "5,6,7,8", "--fft", "2048", "--overlap", "4", "t.wav", "--out",
                                    "t.pan", "--apply"])
    assert args.box == [[1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0]] and args.fft == 2048 and args.overlap == 4 and args.apply
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    out = tmp_path / "t.pan"
    with pytest.raises(SystemExit, match="no CPU fallback"):
        cli.main(["pan", "--box", "1,2,3,4", str(tmp_path / "missing.wav"), "--out", str(out)])
    with pytest.raises(SystemExit, match="no CPU fallback"):
        cli.main(["pan", str(tmp_path / "missing.pan")])
    assert not out.exists()


def test_no_cpu_fallback(tape):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pyaudiorestoration_amd import pypan
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pypan.pan_samples(tape, N.SR, [(0.4, 300.0, 1.0, 4000.0)], 1024, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pypan.apply_pan(tape, N.SR, np.array([[0.0, 1.0], [3.0, 1.0]]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pypan.pan_ratio(np.ones((9, 4), np.float32), np.ones((9, 4), np.float32), [(1, 5, 0, 4)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pypan.process("missing.wav", boxes=[(0.4, 300.0, 1.0, 4000.0)])


def test_pypan_never_imports_the_reference_statements():
    src = open(os.path.join(ROOT, "pyaudiorestoration_amd", "pypan.py")).read()
    assert "oracle" not in src.lower() and "pan_np" not in src and "golden" not in src
    import subprocess
    import sys
    code = "import sys; import pyaudiorestoration_amd.pypan; print(sorted(m for m in sys.modules if m.split('.')[0] == 'oracle'))"
    assert subprocess.check_output([sys.executable, "-c", code], cwd=ROOT, text=True).strip() == "[]"


def test_save_project_writes_the_references_keys(tmp_path):
    import json
    from pyaudiorestoration_amd import pypan
    path = tmp_path / "tape.pan"
    pypan.save_project(str(path), {"fft_size": 4096, "fft_overlap": 8, "fft_zeropad": 1, "source": "tape.wav",
                                   "markers": [pypan.PanSample((1.0, 20.0), (3.0, 40.0), 1.25), (0.5, 1, 0.7, 2, 0.9)]})
    cfg = json.load(open(path))
    assert sorted(cfg) == ["fft_overlap", "fft_size", "fft_zeropad", "markers", "source"]
    assert cfg["markers"] == [[1.0, 20.0, 3.0, 40.0, 1.25], [0.5, 1, 0.7, 2, 0.9]]
    assert open(path).read().startswith('{\n\t"fft_overlap": 8,')                          # indent="\t", sort_keys (util/config.py:21)
