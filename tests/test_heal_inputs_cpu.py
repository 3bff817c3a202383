"""Preconditions of tests/test_heal_kernels_gpu.py, on the CPU: the float64 oracles of tests/heal_inputs.py alone.  The reference's
serial marker loop and the closed form the kernel relies on agree; no cell of any case sits within 1e-6 dB of a clip, so a cell that
differs on the GPU is a kernel error; every named case has the thread geometry it exists for; the two descriptions of the padded
copy source agree.  pytest -s prints the measured figures (NOTES.md, K_heal)."""
import numpy as np
import pytest

import heal_inputs as H


def test_loop_form_equals_closed_form():
    """np.clip(g, previous, 255) marker by marker on a zero (or pre-set) mask == min(255, max(preset, max_k g_k)) to 1e-12 dB"""
    worst = ("", 0.0)
    for c in H.all_cases():
        loop = H.gain_mask_np(c.spec, c.markers, c.preset)
        closed = H.gain_mask_closed_np(c.spec, c.markers, c.preset)
        assert loop.shape == closed.shape == c.spec.shape and np.isfinite(loop).all(), c
        err = float(np.max(np.abs(loop - closed)))
        worst = max(worst, (c.name, err), key=lambda t: t[1])
        assert err <= 1e-12, (c, err)
        # the order of the markers does not matter to the loop either
        back = H.gain_mask_np(c.spec, c.markers[::-1], c.preset)
        assert float(np.max(np.abs(loop - back))) <= 1e-12, c
    print(f"\nloop form against closed form: worst {worst[1]:.2e} dB ({worst[0]})")


def test_margins_at_the_clips():
    """Every box cell's unclipped float64 gain max_k g_k is at least CLIP_MARGIN from 0 and from 255, in every named case and every
    sweep seed: the two float64 evaluations differ by about 1e-13 dB, so neither `written or not` nor `clipped or not` can differ
    legitimately.  No case places a cell exactly at a clip, so nothing is excepted.  A seed that fails is replaced in
    heal_inputs.SWEEP_SEEDS."""
    near0, near255 = {}, {}
    for c in H.all_cases():
        u = H.unclipped_max_np(c.spec, c.markers)
        inside = H.box_cells(c.spec.shape, c.markers)
        assert np.array_equal(inside, np.isfinite(u)), c
        near0[c.name] = float(np.min(np.abs(u[inside])))
        near255[c.name] = float(np.min(np.abs(u[inside] - H.GAIN_MAX)))
    for kind in ("nan", "nan_neg", "inf"):                 # the poison cases: their finite cells
        c, _ = H.poison_case(kind)
        u = H.unclipped_max_np(c.spec, c.markers)
        u = u[np.isfinite(u)]
        near0[c.name], near255[c.name] = float(np.min(np.abs(u))), float(np.min(np.abs(u - H.GAIN_MAX)))
    w0, w255 = min(near0, key=near0.get), min(near255, key=near255.get)
    print(f"\nsmallest distance of an unclipped gain from 0: {near0[w0]:.2e} dB ({w0}); from 255: {near255[w255]:.2e} dB ({w255})")
    bad = {k: (near0[k], near255[k]) for k in near0 if not (near0[k] >= H.CLIP_MARGIN and near255[k] >= H.CLIP_MARGIN)}
    assert not bad, bad


GEOMETRY_KEYS = ("nb", "fs", "nf", "chunks", "nbc", "P", "apply_loops")


@pytest.mark.parametrize("name", H.NAMED)
def test_named_case_has_its_geometry(name):
    c = H.case(name)
    e = c.expect
    assert c.frames <= 96 and c.bins <= 1025
    valid = [m for m in c.markers if H.marker_valid(m, c.frames, c.bins)]
    g = H.kernel_geometry(valid[0])
    for k in GEOMETRY_KEYS:
        if k in e:
            assert g[k] == e[k], (name, k, g[k], e[k])
    fb, fa, fs, bl, bu = valid[0]
    P = g["P"][0]
    if "fs_lt_P" in e:
        assert fs < P                                       # lanes fs .. P - 1 sum no surrounding frame
    if "fs_mod_P" in e:
        assert fs > P and fs % P == e["fs_mod_P"]
    if "nf_lt_P" in e:
        assert 2 < fa - fb < P
    if "nf_mod_P" in e:
        assert fa - fb > P and (fa - fb) % P == e["nf_mod_P"] != 0
    if "start" in e:
        assert fb - fs == 0
    if "end" in e:
        assert fa + fs == c.frames
    if name in ("row257", "row1025"):
        assert (bl, bu) == (0, c.bins)
    u = H.unclipped_max_np(c.spec, c.markers)
    inside = H.box_cells(c.spec.shape, c.markers)
    if e.get("all_clipped"):
        assert np.all(u[inside] > H.GAIN_MAX) and np.all(np.abs(np.asarray(c.spec)[fa:fa + fs]) >= 1e6)
        box = np.abs(np.asarray(c.spec)[fb:fa])
        assert np.all(box == 0) if e["box"] == 0 else np.all((box >= 1e-9) & (box <= 2.1e-9))
    if e.get("none_written"):
        assert np.all(u[inside] < 0) and not np.any(H.gain_mask_np(c.spec, c.markers))
    if e.get("preset"):
        new = H.gain_mask_np(c.spec, c.markers)
        pre = np.asarray(c.preset, dtype=np.float64)
        assert np.any((pre > new) & inside) and np.any((pre > 0) & (pre < new)) and np.any((pre > 0) & ~inside)
        assert np.array_equal(H.gain_mask_np(c.spec, c.markers, c.preset), np.maximum(pre, new))
    if e.get("overlap"):
        count = sum(H.box_cells(c.spec.shape, [m]).astype(int) for m in c.markers)
        assert count.max() >= 3 and len({m[4] - m[3] for m in c.markers}) == len(c.markers)
        f0, f1, _, b0, b1 = c.markers[0]
        f2, f3, _, b2, b3 = c.markers[1]
        assert f0 <= f2 and f3 <= f1 and b0 <= b2 and b3 <= b1                      # the second box nested in the first
        m = H.gain_mask_np(c.spec, c.markers)
        assert np.any(m[inside] > 0) and np.any(m[inside] == 0)                     # gains of both signs
    if e.get("twice"):
        assert c.markers[0] == c.markers[1]
    if "markers" in e:
        assert len(valid) == len(c.markers) == e["markers"]
        m = H.gain_mask_np(c.spec, c.markers)
        assert np.any(m[inside] > 0) and np.any(m[inside] == 0)
    if "invalid" in e:
        assert len(valid) == e["valid"] and len(c.markers) - len(valid) == e["invalid"]
        fr, bn = c.frames, c.bins
        assert any(m[0] - m[2] == -1 for m in c.markers) and any(m[1] + m[2] == fr + 1 for m in c.markers)
        assert any(m[3] == -1 for m in c.markers) and any(m[4] == bn + 1 for m in c.markers)
        assert any(m[1] == m[0] for m in c.markers) and any(m[2] == 0 for m in c.markers)
        assert any(m[4] == m[3] for m in c.markers) and any(m[4] < m[3] for m in c.markers)
        assert H.max_fs(c) + 2 <= 12                       # what the GPU file's guard rows must cover


def test_sweep_reaches_both_signs_and_many_geometries():
    assert len(set(H.SWEEP_SEEDS)) == 24
    pos = neg = 0
    Ps, chunked = set(), 0
    for seed in H.SWEEP_SEEDS:
        c = H.sweep_case(seed)
        assert all(H.marker_valid(m, c.frames, c.bins) for m in c.markers), c
        u = H.unclipped_max_np(c.spec, c.markers)
        inside = np.isfinite(u)
        pos += int(np.sum(u[inside] > 0))
        neg += int(np.sum(u[inside] < 0))
        for m in c.markers:
            g = H.kernel_geometry(m)
            Ps.update(g["P"])
            chunked += g["chunks"] > 1
    print(f"\nsweep: {pos} cells with a positive gain, {neg} with a negative one, P in {sorted(Ps)}, {chunked} boxes over 256 bins")
    assert pos >= 1000 and neg >= 1000 and len(Ps) >= 5 and chunked >= 3


def test_poison_values_in_the_reference():
    """What the GPU test expects of the reference: a NaN in one surrounding frame of one bin makes every box cell of that bin NaN,
    whether the overlapping marker comes before or after; an Inf gives [255, ..., 255, NaN] (inf * 0 at the box's last frame).
    Every other bin is finite: this restatement does not interpolate along bins."""
    for kind in ("nan", "nan_neg"):
        c, b = H.poison_case(kind)
        assert np.isnan(c.spec[8, b])
        for ms in (c.markers, c.markers[::-1]):
            m = H.gain_mask_np(c.spec, ms)
            assert np.isnan(m[10:16, b]).all()
            assert np.isfinite(np.delete(m, b, axis=1)).all() and np.isfinite(m[16:, b]).all()
    c, b = H.poison_case("inf")
    for ms in (c.markers, c.markers[::-1]):
        m = H.gain_mask_np(c.spec, ms)
        assert np.array_equal(m[10:15, b], np.full(5, 255.0)) and np.isnan(m[15, b])
        assert np.isfinite(np.delete(m, b, axis=1)).all()


# ------------------------------------------------------------------------------------------ the other four oracles
@pytest.mark.parametrize("name", H.COPY_CASES)
def test_copy_source_two_descriptions_agree(name):
    c = H.copy_case(name)
    assert c.total == int(c.lens.sum()) and np.array_equal(c.run_start, np.cumsum(c.lens) - c.lens)
    a = H.copy_segments_np(c)
    # no two segments write the same sample, every written sample lies inside the destination
    hits = np.zeros(c.dst_len, dtype=int)
    for d0, ln in zip(c.dst_start, c.lens):
        assert 0 <= d0 and d0 + ln <= c.dst_len
        hits[d0:d0 + ln] += 1
    assert hits.max(initial=0) <= 1 and np.array_equal(a != H.SENTINEL, hits == 1)
    if c.padded:
        b = H.copy_segments_np(c, source=H.padded_source_periodic)
        assert np.array_equal(a, b)
    else:
        assert all(0 <= s0 and s0 + ln <= len(c.src) for s0, ln in zip(c.src_start, c.lens))


def test_reflect_period_equals_np_pad():
    """numpy's reflect with a pad longer than the array is the periodic map of period 2 (n - 1)"""
    for n in (1, 2, 5, 37):
        x = np.arange(n, dtype=np.float32) + 1
        q = np.arange(-4 * n - 3, 5 * n + 4)
        assert np.array_equal(H.padded_source_np(x, n, n, q), x[H.reflect_index(q, n)])


def test_copy_cases_reach_the_walk():
    """forty segments inside one 2048-sample span; a segment across a span boundary; zero lengths first, in the middle and last"""
    c = H.copy_case("forty_short")
    assert len(c.lens) == 40 and c.total < H.K_COPY_SPAN and c.lens.max() < 256
    c = H.copy_case("straddle")
    ends = c.run_start + c.lens
    assert np.any((c.run_start < H.K_COPY_SPAN) & (ends > H.K_COPY_SPAN))
    c = H.copy_case("zero_lengths")
    assert c.lens[0] == 0 and c.lens[-1] == 0 and np.any(c.lens[1:-1] == 0)
    assert [H.copy_case(f"total{t}").total for t in (2047, 2048, 2049, 1)] == [2047, 2048, 2049, 1]
    c = H.copy_case("pad_periods_valid5")
    assert c.n_padded == 5 and c.src_start.min() == -12 and (c.src_start + c.lens).max() == 17


def test_curve_scale_oracle_is_finite_and_bounded():
    for n, frames in H.CURVE_SHAPES:
        for n_ch, stride in H.CHANNELS:
            sig, fac = H.curve_case(n, frames, n_ch, stride)
            ref = H.curve_scale_np(sig, fac)
            bound = H.curve_scale_bound(sig, fac)
            assert ref.shape == bound.shape == (n_ch, n) and np.isfinite(ref).all() and np.isfinite(bound).all()
            # the bound scales with the operand: it is never below one rounding of the result
            assert np.all(bound >= 2.0 ** -53 * np.abs(ref))
    sig, fac = H.curve_case(97, 97, 2, 2)
    assert np.array_equal(H.curve_scale_np(sig, fac), sig[:, :2].T.astype(np.float64) * fac)         # every sample on a knot


def test_accumulate_oracle_rounds_ties_to_even():
    sig, y = H.accumulate_case(13, 2, 3)
    out = H.accumulate_np(sig, y)
    one, nxt = np.float32(1), np.nextafter(np.float32(1), np.float32(2))
    assert out[0, 0] == one and out[1, 0] == np.nextafter(nxt, np.float32(2)) and out[2, 1] == -one
    assert np.array_equal(out[:, 2], sig[:, 2])                                                      # the stride's spare column


def test_band_mean_oracle_special_values():
    mag = H.band_mag(3, 6, 70).copy()
    mag[1, 5], mag[2, 6], mag[3, 7] = 0.0, np.nan, np.float32(1e-40)
    with np.errstate(all="ignore"):
        out = H.band_mean_db_np(mag, 0, 70, 0, 6)
    assert out[1] == -np.inf and np.isnan(out[2]) and np.isfinite(out[[0, 3, 4, 5]]).all()
