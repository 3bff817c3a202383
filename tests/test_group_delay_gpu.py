"""group_delay.measure on the GPU against the reference's recorded run (tests/golden/group_delay.npz) and the per-band float64 statement
of tests/group_delay_np.py.  Every band is held to azimuth_inputs.flow_bounds' formula with windows of ones; the filter's share per band
is the existing pin of K_sosfiltfilt, filt_inputs.R x max(scipy's error against filt_np's compensated blocked statement, FLOOR), computed
on the CPU for that band and signal.  pytest -s prints the measured figures."""
import functools
import json
import os
import warnings

import numpy as np
import pytest

import group_delay_np as G
import xcorr_inputs as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def GD():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pyaudiorestoration_amd import group_delay
    return group_delay


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_result(r1, r2, levels=True):
    names = ("band_centers", "lags", "correlations", "lags_all", "correlations_all") + (("magnitudes", "levels_ref", "levels_src") if levels else ())
    return np.array_equal(r1.kept, r2.kept) and all(np.array_equal(bits(getattr(r1, k)), bits(getattr(r2, k))) for k in names)


def band_bounds(band, ref, src):
    """((lag bound, corr bound), (level tolerance ref, src)) of one band of measure_np on the signals ref, src (in their own dtype)"""
    tol_a = tol_b = 0.0
    if band.sos is not None:
        tol_a, tol_b = G.filter_tolerance(band.sos, ref, band.ya), G.filter_tolerance(band.sos, src, band.yb)
    flow = G.bounds(band.oracle, len(band.yb), G.row_eps(tol_a, band.ya), G.row_eps(tol_b, band.yb))
    # a level is ||y|| / sqrt(n): the filter moves ||y|| by at most tol max |y| sqrt(n), the norm's sum rounds by 2 n u
    level = [tol * np.max(np.abs(y)) + 2.0 * len(y) * X.U * lv for tol, y, lv in ((tol_a, band.ya, band.level_ref), (tol_b, band.yb, band.level_src))]
    return flow, level


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "group_delay.npz"))
    ref, src, sr = g["ref"], g["src"], int(g["sr"])
    # float32 signals: scipy extends them in float32 for the reference, and so does group_delay.measure (measure_np's widen=False)
    bands = G.measure_np(ref, src, sr, g["band_limits"])
    return g, ref, src, sr, bands, [band_bounds(b, ref, src) for b in bands]


@pytest.fixture(scope="module")
def measured(GD):
    g, ref, src, sr, _, _ = fixture()
    return GD.measure(ref, src, sr)


def check_bands(res, bands, allowed, what):
    worst = [0.0, 0.0]
    for k, (b, ((bd, bc), (la, lb))) in enumerate(zip(bands, allowed)):
        assert abs(res.lags_all[k] - b.lag) <= bd and abs(res.correlations_all[k] - b.corr) <= bc, \
            (what, k, b.lo, b.hi, res.lags_all[k] - b.lag, bd, res.correlations_all[k] - b.corr, bc)
        assert abs(res.levels_ref[k] - b.level_ref) <= la and abs(res.levels_src[k] - b.level_src) <= lb, (what, k)
        worst = [max(worst[0], abs(res.lags_all[k] - b.lag) / bd), max(worst[1], abs(res.correlations_all[k] - b.corr) / bc)]
    print(f"\n{what}: worst share of the bound over {len(bands)} bands: lag {worst[0]:.3f}, corr {worst[1]:.3f}", end="")


def test_measure_against_the_oracle_and_the_references_run(GD, measured):
    g, ref, src, sr, bands, allowed = fixture()
    res = measured
    assert np.array_equal(res.band_lo, g["band_limits"][:-1]) and np.array_equal(res.band_hi, g["band_limits"][1:])
    assert np.array_equal(res.band_centers, g["band_centers"])                     # the kept set is the reference's
    assert np.array_equal(res.kept, np.array([b.corr > G.MIN_CORR for b in bands]))
    assert len(res.lags_all) == len(bands) == 43 and res.kept.sum() == 42
    check_bands(res, bands, allowed, "fixture")                                    # every band, the rejected one included
    kept = np.flatnonzero(res.kept)
    for j, k in enumerate(kept):
        (_, _), (la, lb) = allowed[k]
        assert abs(res.magnitudes[j] - g["magnitudes"][j]) <= la + lb + 4 * X.U * (res.levels_ref[k] + res.levels_src[k]), k
        assert res.magnitudes[j] == res.levels_ref[k] - res.levels_src[k] and res.lags[j] == res.lags_all[k]
    rep = GD.report(res)
    assert rep["n_bands"] == 43 and rep["n_kept"] == 42 and len(rep["lags"]) == 42 and json.dumps(rep)


def test_the_same_bounds_hold_against_the_golden_lists(GD, measured):
    """The kept bands' lags and correlations against the reference's recorded lists, under the bounds of the test above.  The lists
    were recorded from float32 signals, which scipy extends in float32 before it filters: with the extension widened first, 12-14 Hz
    missed its correlation bound (1.111e-09 of 1.063e-09), so group_delay.measure extends as scipy does."""
    g, ref, src, sr, bands, allowed = fixture()
    res = measured
    miss = []
    for j, k in enumerate(np.flatnonzero(res.kept)):
        (bd, bc), _ = allowed[k]
        dl, dc = abs(res.lags[j] - g["lags"][j]), abs(res.correlations[j] - g["correlations"][j])
        print(f"\nband {k}: lag off by {dl:.3e} of {bd:.3e}, corr off by {dc:.3e} of {bc:.3e}", end="")
        if not (dl <= bd and dc <= bc):
            miss.append((int(k), dl, bd, dc, bc))
    assert not miss, miss


def test_batched_equals_the_loop_and_a_hand_composition(GD, measured):
    import torch
    from pyaudiorestoration_amd import correlation, filters
    g, ref, src, sr, bands, allowed = fixture()
    loop = GD.measure(ref, src, sr, batched=False)
    assert same_result(measured, GD.measure(ref, src, sr, batched=True))
    assert same_result(measured, loop, levels=False)
    for k, (_, (la, lb)) in enumerate(allowed):                                    # the loop's norms are summed in another order
        assert abs(loop.levels_ref[k] - measured.levels_ref[k]) <= la and abs(loop.levels_src[k] - measured.levels_src[k]) <= lb
    # the hand composition on float64 signals, whose extension K_sosfiltfilt forms itself
    measured64 = GD.measure(ref.astype(np.float64), src.astype(np.float64), sr)
    lo, hi = g["band_limits"][:-1].astype(np.float64), g["band_limits"][1:].astype(np.float64)
    x = torch.stack([torch.from_numpy(ref.astype(np.float64)).cuda()] * 43 + [torch.from_numpy(src.astype(np.float64)).cuda()] * 43)
    y = filters.bandpass_batch_dev(x, np.tile(lo, 2), np.tile(hi, 2), sr, 1)
    for k in range(43):
        d, c = correlation.find_delay(y[k], y[43 + k])
        assert bits(-d) == bits(measured64.lags_all[k]) and bits(c) == bits(measured64.correlations_all[k]), k


def test_chunks_sections_and_input_kinds_change_nothing(GD, measured):
    import torch
    g, ref, src, sr, _, _ = fixture()
    assert same_result(measured, GD.measure(ref, src, sr, max_bytes=1))            # one band per chunk, one row per pass
    assert same_result(measured, GD.measure(ref, src, sr, section=12))
    assert same_result(measured, GD.measure(torch.from_numpy(ref).cuda(), torch.from_numpy(src).cuda(), sr))
    ref64, src64 = ref.astype(np.float64), src.astype(np.float64)
    res64 = GD.measure(ref64, src64, sr)                                           # float64 in: the extension is float64's
    assert same_result(res64, GD.measure(ref64, torch.from_numpy(src64).cuda(), sr))
    bands64 = G.measure_np(ref, src, sr, g["band_limits"], widen=True)
    check_bands(res64, bands64, [band_bounds(b, ref64, src64) for b in bands64], "float64 input")


def test_time_span(GD):
    g, ref, src, sr, _, _ = fixture()
    t0, t1 = 0.2003, 1.2001
    s0, s1 = int(t0 * sr), int(t1 * sr)
    res = GD.measure(ref, src, sr, t0=t0, t1=t1, f_lower=40)
    assert same_result(res, GD.measure(ref[s0:s1], src[s0:s1], sr, f_lower=40))
    bands = G.measure_np(ref, src, sr, GD.band_limits(40), t0=t0, t1=t1)
    check_bands(res, bands, [band_bounds(b, ref[s0:s1], src[s0:s1]) for b in bands], "t0, t1")
    with pytest.raises(ValueError, match="empty span"):
        GD.measure(ref, src, sr, t0=1.0, t1=1.0)


def last_lag_pair(n=20000, seed=5):
    """`b` is `a` advanced by n/2 - 1 samples: every band's correlation peaks on the last lag of the 'same' span"""
    rng = np.random.default_rng([92, seed])
    a = rng.standard_normal(n)
    b = 1e-3 * rng.standard_normal(n)
    b[:n // 2 + 1] += a[n // 2 - 1:]
    return a, b


def test_strict_on_both_sides(GD):
    a, b = last_lag_pair()
    kw = dict(sr=8000, f_lower=200, f_upper=2000, bandwidth=300)
    bands = G.measure_np(a, b, 8000, GD.band_limits(200, 2000, 300))
    assert len(bands) == 5 and all(band.status == 1 for band in bands)             # the precondition, by the float64 statement
    with pytest.raises(IndexError, match=r"band 0, 199 \.\. 316 Hz"):
        GD.measure(a, b, **kw)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = GD.measure(a, b, strict=False, **kw)
    assert len(caught) == 5 and not res.kept.any() and np.all(np.isnan(res.lags_all)) and len(res.lags) == 0
    assert np.all(np.isfinite(res.levels_ref)) and np.all(res.levels_ref > 0)


def test_band_edges_above_nyquist(GD):
    """sr = 3000 Hz: the bands up to 1381 Hz are band-passes, 1381 .. 1563 Hz has only its lower edge inside (0, Nyquist) -- a
    high-pass, another cascade shape -- and the two bands above take the unfiltered rows, as the reference's filter returns its input"""
    g, ref, src, _, _, _ = fixture()
    sr, n = 3000, 20001
    ref, src = ref[:n], src[:n]
    res = GD.measure(ref, src, sr)
    bands = G.measure_np(ref, src, sr, GD.band_limits())
    assert [b.sos is None for b in bands[-3:]] == [False, True, True] and bands[-3].sos.shape[0] == 1
    check_bands(res, bands, [band_bounds(b, ref, src) for b in bands], "sr 3000")
    assert bits(res.lags_all[-1]) == bits(res.lags_all[-2]) and bits(res.levels_src[-1]) == bits(res.levels_src[-2])
    assert same_result(res, GD.measure(ref, src, sr, batched=False), levels=False)


def test_measure_file_and_cli(GD, tmp_path, measured):
    from pyaudiorestoration_amd import cli, io_ops
    g, ref, src, sr, _, _ = fixture()
    # the golden take is a one-channel file: its channel against itself is lag 0 at correlation 1 in every band
    flac = os.path.join(ROOT, "tests", "golden", "dropouts_sample.flac")
    res = GD.measure_file(flac, ref_channel=0, src_channel=0)
    assert res.kept.all() and np.all(np.abs(res.lags_all) <= 1e-6) and np.all(np.abs(res.correlations_all - 1.0) <= 1e-9)
    assert np.all(res.magnitudes == 0.0)
    with pytest.raises(ValueError, match="1 channel"):
        GD.measure_file(flac, ref_channel=0, src_channel=1)
    out = str(tmp_path / "mono.json")
    assert cli.main(["groupdelay", flac, "--ref", flac, "--json", out]) == 0
    rep = json.load(open(out))
    assert rep["n_kept"] == 43 and rep["lags_all"] == res.lags_all.tolist() and rep["sr"] == 44100
    # two channels of one file: the fixture's pair as a float WAV
    wav = str(tmp_path / "pair.wav")
    io_ops.write_wav_float(wav, np.stack((ref, src), axis=-1), sr)
    assert same_result(measured, GD.measure_file(wav))
    assert same_result(GD.measure(src, ref, sr), GD.measure_file(wav, ref_channel=1, src_channel=0))
    out2 = str(tmp_path / "pair.json")
    assert cli.main(["groupdelay", wav, "--json", out2, "--min-corr", "0.6", "--bands", "10,2000,45"]) == 0
    rep2 = json.load(open(out2))
    assert rep2["n_kept"] == 42 and rep2["lags"] == measured.lags.tolist() and rep2["kept"] == measured.kept.tolist()
    out3 = str(tmp_path / "span.json")
    assert cli.main(["groupdelay", wav, "--range", "0.2,1.2", "--bands", "40,2000,45", "--json", out3]) == 0
    assert json.load(open(out3))["lags_all"] == GD.measure(ref, src, sr, f_lower=40, t0=0.2, t1=1.2).lags_all.tolist()
