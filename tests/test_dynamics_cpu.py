"""The dynamics matcher without a GPU: tests/dynamics_np.py restates the reference (bit for bit at the fixture's samples), its
exact-sum variants agree with it, the reflect index map is scipy's, the input builders of the GPU tests hit the cases they claim,
the new entry points refuse bad arguments before any device call, and the Python layer raises what it documents."""
import ctypes

import numpy as np
import pytest
import scipy.ndimage

import dynamics_np as D


@pytest.fixture(scope="module")
def golden_case():
    g = np.load(D.GOLDEN)
    src, ref = D.golden_input(g)
    stages = []
    facs = D.gain_curves_np(src, ref, int(g["sr"]), stages=stages)
    return dict(g=g, src=src, ref=ref, facs=facs, stages=stages, out=D.apply_np(src, facs, D.HOP))


def test_restatement_equals_the_reference_bit_for_bit(golden_case):
    g, out = golden_case["g"], golden_case["out"]
    rows = D.golden_rows(len(out))
    assert g["out"].dtype == np.float64 and g["out"].shape == (len(rows), 2)
    assert np.array_equal(out[rows].view(np.uint64), g["out"].view(np.uint64))
    assert float(g["out_peak"]) == np.max(np.abs(out))
    # the fixture covers what it is there for: a gain above and below 1, the clip at 2, and the overlap-add's tail
    facs = golden_case["facs"]
    assert facs.max() == 2.0 and facs.min() < 0.5 and np.all(np.isfinite(facs))
    F, ch = facs.shape[1], D.CORR_SZ // 2
    x_last = ch * ((F - 1) // ch)
    al = golden_case["stages"][0]["aligned"]
    assert x_last == 4096 and np.all(al[x_last - 1:] == 0) and np.all(al[x_last - ch:x_last - 1] != 0)
    assert np.array_equal(facs[0][x_last:], np.minimum(np.power(10, golden_case["stages"][0]["b"][x_last:]), 2.0))


def test_golden_input_reaches_the_floor_and_ends_on_a_one_sample_frame(golden_case):
    src = golden_case["src"]
    n = len(src)
    assert n % D.HOP == 1
    y = D.bandpass_np(src[:, 0], D.LOWER, D.UPPER, D.SR)
    rms = D.windowed_rms_np(y, D.HOP, D.SZ)
    assert len(rms) == D.n_frames(n, D.HOP) and rms[-1] == abs(y[-1])
    assert np.any(rms < D.FLOOR) and np.any(rms > 100 * D.FLOOR)
    quiet = np.flatnonzero(np.all(src == 0, axis=1))
    assert len(quiet) >= 2000 > D.SZ                                 # the silent stretch (what the roll leaves of it in both channels)


def test_exact_variants_agree_with_the_restatement(golden_case):
    """the oracles the device is measured against compute what the reference computes: swapped into the restatement, stage by
    stage, they move the output by less than 1e-12 of its peak"""
    src, ref, sr = golden_case["src"], golden_case["ref"], D.SR
    ns = int(sr * D.SMOOTHING_SEC / D.HOP)
    facs = []
    for c in range(2):
        a, _ = D.log_curve_exact(D.bandpass_np(src[:, c], D.LOWER, D.UPPER, sr), D.HOP, D.SZ)
        b, _ = D.log_curve_exact(D.bandpass_np(ref[:, c], D.LOWER, D.UPPER, sr), D.HOP, D.SZ)
        b = D.level_match_exact(a, b)
        a, b = D.uniform_reflect_exact(a, ns)[0], D.uniform_reflect_exact(b, ns)[0]
        facs.append(D.fac_np(b, D.aligned_np(a, D.CORR_SZ)))
    out = D.apply_np(src, np.asarray(facs), D.HOP)
    err = np.max(np.abs(out - golden_case["out"])) / np.max(np.abs(golden_case["out"]))
    print("exact-sum variants against the restatement:", err, "of the peak")
    assert err < 1e-12


@pytest.mark.parametrize("size", [110, 7, 1200])
def test_reflect_index_map_is_scipys(size):
    x = D.box_row(500)
    want = scipy.ndimage.uniform_filter1d(x, size=size)
    got, peak = D.uniform_reflect_exact(x, size)
    assert np.max(np.abs(got - want)) < 1e-14
    assert np.all(peak <= np.max(np.abs(x))) and np.all(peak >= np.abs(x))


def test_fac_oracle_agrees_with_numpy():
    a, b = D.fac_rows(75, 16)
    al = D.aligned_np(a, 16)
    want, hard = D.fac_exact(b, al)
    got = D.fac_np(b, al)
    assert hard.any() and (~hard).any() and want[75 // 3] == 0.0 and got[75 // 3] == 0.0
    assert np.array_equal(got[hard], want[hard])
    assert np.all(np.abs(got[~hard] - want[~hard]) <= 4 * D.U * want[~hard])       # numpy's 10**x is within 1.1 units here


def test_input_builders_hit_what_they_claim():
    # K_wrms: a last frame of one sample, frames on both sides of the floor and inside the silent stretch
    assert 301 % 4 == 1 and 4099 % 32 == 3 and 301 % 32 == 13 and 301 < 400
    n, hop, sz = 4099, 32, 512
    x = D.floor_row(n, hop, sz)
    _, r = D.log_curve_exact(x, hop, sz)
    assert np.any(r > 2 * D.FLOOR) and np.any((r < D.FLOOR) & (r > 0)) and np.any((r > D.FLOOR) & (r < 1.5 * D.FLOOR))
    silent = np.flatnonzero(x == 0)
    assert len(silent) > sz and np.any(r == 0)
    # K_level: the level curves keep |b - mean b| <= |value| (dynamics_np.level_bound)
    for rows in (1, 4):
        for F in (1, 75, 4097):
            a, b = D.level_rows(rows, F)
            for ar, br in zip(a, b):
                assert np.all(np.abs(br - np.mean(br)) <= np.abs(D.level_match_exact(ar, br)))
    # K_dynfac: F in each of {<= corr_hop, corr_hop + 1, k corr_hop, k corr_hop + 1}
    ch = 8
    assert [F <= ch for F in (8, 9, 24, 25, 75)] == [True, False, False, False, False]
    assert 9 == ch + 1 and 24 % ch == 0 and 25 % ch == 1 and 75 % ch == 3
    for F in (8, 9, 24, 25, 75):
        a, b = D.fac_rows(F, 16)
        al = D.aligned_np(a, 16)
        x_last = ch * ((F - 1) // ch)
        assert np.all(al[max(x_last - 1, 0):] == 0)
        if F <= ch:
            assert np.all(al == 0)
        else:
            assert np.all(al[:x_last - 1] != 0)
        fac, hard = D.fac_exact(b, al)
        assert np.isnan(b[F // 3]) and fac[F // 3] == 0.0
        if F >= 24:
            assert np.any(fac == 2.0) and np.any((fac > 0) & (fac < 2.0))
    # K_dynapply: the hold after the last key runs over 0 and hop - 1 samples
    for hop in (1, 32):
        F = 5
        assert D.n_frames((F - 1) * hop + 1, hop) == F and D.n_frames(F * hop, hop) == F


def test_aligned_formula_of_the_kernel_is_the_references_loop():
    """k_dynfac's closed form (two products, added in window order, the first onto 0.0) against the padded loop, bit for bit"""
    for corr_sz, F in ((16, 8), (16, 9), (16, 24), (16, 25), (16, 75), (4096, 6250)):
        a, _ = D.fac_rows(F, corr_sz)
        ch, hann = corr_sz // 2, np.hanning(corr_sz)
        K = (F - 1) // ch
        i = np.arange(F)
        k1, m = i // ch + 1, i % ch
        al = np.zeros(F)
        al = np.where(k1 <= K, al + a * hann[m + ch], al)
        al = np.where(k1 + 1 <= K, al + a * hann[m], al)
        assert np.array_equal(al.view(np.uint64), D.aligned_np(a, corr_sz).view(np.uint64)), (corr_sz, F)


def test_entry_points_reject_bad_arguments_before_any_device_call():
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(64)
    q = ctypes.c_void_p(128)

    def refused(rc, *words, code=1):
        msg = _lib.last_error()
        assert rc == code, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)
    name = "par_windowed_rms_log10_f64"
    refused(L.par_windowed_rms_log10_f64(0, None, 100, 1, 100, 32, 512, 0.0005, 1, q, None), name, "null")
    refused(L.par_windowed_rms_log10_f64(0, p, 100, 1, 100, 32, 512, 0.0005, 1, None, None), name, "null")
    refused(L.par_windowed_rms_log10_f64(0, p, 100, 0, 100, 32, 512, 0.0005, 1, q, None), name, "rows 0")
    refused(L.par_windowed_rms_log10_f64(0, p, 100, 1, 0, 32, 512, 0.0005, 1, q, None), name, "n 0")
    refused(L.par_windowed_rms_log10_f64(0, p, 100, 1, 100, 0, 512, 0.0005, 1, q, None), name, "hop 0")
    refused(L.par_windowed_rms_log10_f64(0, p, 100, 1, 100, 32, 0, 0.0005, 1, q, None), name, "sz 0")
    refused(L.par_windowed_rms_log10_f64(0, p, 99, 2, 100, 32, 512, 0.0005, 1, q, None), name, "x_pitch 99")
    refused(L.par_windowed_rms_log10_f64(0, p, 100, 1, 100, 32, 512, float("nan"), 1, q, None), name, "NaN")
    name = "par_level_match_f64"
    refused(L.par_level_match_f64(0, None, p, 1, 10, q, None), name, "null")
    refused(L.par_level_match_f64(0, p, None, 1, 10, q, None), name, "null")
    refused(L.par_level_match_f64(0, p, q, 1, 10, None, None), name, "null")
    refused(L.par_level_match_f64(0, p, q, 0, 10, q, None), name, "rows 0")
    refused(L.par_level_match_f64(0, p, q, 1, 0, q, None), name, "F 0")
    refused(L.par_level_match_f64(0, p, q, 1, 10, p, None), name, "out_b is a")
    name = "par_uniform_filter_reflect_f64"
    refused(L.par_uniform_filter_reflect_f64(0, None, 1, 10, 3, q, None), name, "null")
    refused(L.par_uniform_filter_reflect_f64(0, p, 1, 10, 3, None, None), name, "null")
    refused(L.par_uniform_filter_reflect_f64(0, p, 1, 10, 3, p, None), name, "in place")
    refused(L.par_uniform_filter_reflect_f64(0, p, 0, 10, 3, q, None), name, "rows 0")
    refused(L.par_uniform_filter_reflect_f64(0, p, 1, 0, 3, q, None), name, "n 0")
    refused(L.par_uniform_filter_reflect_f64(0, p, 1, 10, 0, q, None), name, "size 0")
    name = "par_dynamics_factor_f64"
    refused(L.par_dynamics_factor_f64(0, None, p, 1, 10, p, 16, None, q, None), name, "null")
    refused(L.par_dynamics_factor_f64(0, p, None, 1, 10, p, 16, None, q, None), name, "null")
    refused(L.par_dynamics_factor_f64(0, p, p, 1, 10, None, 16, None, q, None), name, "null")
    refused(L.par_dynamics_factor_f64(0, p, p, 1, 10, p, 16, None, None, None), name, "null")
    refused(L.par_dynamics_factor_f64(0, p, p, 0, 10, p, 16, None, q, None), name, "rows 0")
    refused(L.par_dynamics_factor_f64(0, p, p, 1, 0, p, 16, None, q, None), name, "F 0")
    refused(L.par_dynamics_factor_f64(0, p, p, 1, 10, p, 15, None, q, None), name, "corr_sz 15")
    refused(L.par_dynamics_factor_f64(0, p, p, 1, 10, p, 0, None, q, None), name, "corr_sz 0")
    name = "par_dynamics_apply_f32"
    refused(L.par_dynamics_apply_f32(0, None, 2, 2, 100, p, 4, 32, q, 2, None), name, "null")
    refused(L.par_dynamics_apply_f32(0, p, 2, 2, 100, None, 4, 32, q, 2, None), name, "null")
    refused(L.par_dynamics_apply_f32(0, p, 2, 2, 100, p, 4, 32, None, 2, None), name, "null")
    refused(L.par_dynamics_apply_f32(0, p, 2, 2, 100, p, 4, 32, p, 2, None), name, "in place")
    refused(L.par_dynamics_apply_f32(0, p, 2, 2, 0, p, 4, 32, q, 2, None), name, "n 0")
    refused(L.par_dynamics_apply_f32(0, p, 2, 2, 100, p, 4, 0, q, 2, None), name, "hop 0")
    refused(L.par_dynamics_apply_f32(0, p, 2, 0, 100, p, 4, 32, q, 2, None), name, "channels 0")
    refused(L.par_dynamics_apply_f32(0, p, 1, 2, 100, p, 4, 32, q, 2, None), name, "stride")
    refused(L.par_dynamics_apply_f32(0, p, 2, 2, 100, p, 4, 32, q, 1, None), name, "stride")
    refused(L.par_dynamics_apply_f32(0, p, 2, 2, 100, p, 3, 32, q, 2, None), name, "F 3", "4 frames")
    refused(L.par_dynamics_apply_f32(0, p, 9, 9, 100, p, 4, 32, q, 9, None), name, "9 channels", code=3)
    with pytest.raises(_lib.ParUnsupported):
        _lib.check(3)
    assert L.par_version() == 109                                    # the entry points are added at ABI 109


def test_python_layer_raises_what_it_documents(tmp_path):
    from pyaudiorestoration_amd import decompressor as P, io_ops
    x2, x1 = np.zeros((1000, 2), np.float32), np.zeros((1000, 1), np.float32)
    with pytest.raises(ValueError, match="amount of channels"):
        P.match_dynamics(x2, x1, D.SR)
    with pytest.raises(ValueError, match="at least 1"):
        P.gain_curves(x2, x2, 300)                                   # int(300 * 0.08 / 32) == 0: scipy refuses a size of 0
    with pytest.raises(ValueError, match="at least 1"):
        P.match_dynamics(x2, x2, D.SR, smoothing_sec=0.0)
    with pytest.raises(RuntimeError):
        scipy.ndimage.uniform_filter1d(np.zeros(10), size=0)
    assert P.smoothing_size(D.SR, 0.08, 32) == 110 and P.n_frames(140001, 32) == 4376 and P.n_frames(64, 32) == 2
    a, b, c = (str(tmp_path / f) for f in ("a.wav", "b.wav", "c.wav"))
    io_ops.write_wav_float(a, x2, 44100)
    io_ops.write_wav_float(b, x2, 48000)
    io_ops.write_wav_float(c, x1, 44100)
    with pytest.raises(ValueError, match="sample rate"):
        P.process(a, b)
    with pytest.raises(ValueError, match="amount of channels"):
        P.process(a, c)
    from pyaudiorestoration_amd import cli
    args = cli.parser().parse_args(["dynamics", "src.wav", "ref.wav"])
    assert args.cmd == "dynamics" and args.src == "src.wav" and args.ref == "ref.wav"
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["dynamics", "only_one.wav"])
