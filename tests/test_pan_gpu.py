"""The stereo balance kernels at the C ABI and pypan.py end to end, on the GPU.  Statements and bounds: tests/pan_np.py.

Entry 1 (par_pan_ratio_f32): count exact, fac within B_ratio of math.fsum over numpy's float32 quotients of the same magnitudes.
Entry 2 (par_stft_pan_ratio_f32): against entry 1 on par_stft_f32 mode-1 output of the same samples, same count, within B_fused.
Entry 3 (par_pan_apply_f32): numpy bit for bit.  End to end: the fixture the reference computed, under B_ref.
Every output lies between sentinel cells that must stay untouched, and every call is made twice: the runs agree bit for bit."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import pan_np as N
import stft_np as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def par():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    from pyaudiorestoration_amd import _dev, _lib

    class P:
        pass
    p = P()
    p.torch, p.dev, p.L, p.check, p.stream = torch, 0, _lib.lib(), _lib.check, lambda: _dev.stream_ptr(0)
    return p


@pytest.fixture(scope="module")
def g(golden):
    return golden["pypan"]


@pytest.fixture(scope="module")
def tape():
    return N.stereo_tape()


def _boxes(par, cells):
    host = np.ascontiguousarray(np.asarray(cells, dtype=np.int32).reshape(-1, 4))
    return host, par.torch.from_numpy(host.copy()).cuda()


def _outputs(par, n_box):
    return S.Guarded(par.torch, 2 * n_box), S.Guarded(par.torch, 2 * n_box)


def _read(par, fac, cnt, scratch):
    par.torch.cuda.synchronize()
    f, ok_f = fac.read()
    c, ok_c = cnt.read()
    assert ok_f and ok_c and scratch.read()[1], "guards"
    return f.copy().view(np.float64), c.copy().view(np.int64)


def run_ratio(par, L, R, bins, cells, short=False):
    """L, R: float32 [frames][pitch] -> (fac, count) of one guarded call, made twice"""
    frames, pitch = L.shape
    host, dev_boxes = _boxes(par, cells)
    nb = len(host)
    need = int(par.L.par_pan_ratio_scratch_bytes(host.ctypes.data, nb))
    assert need >= 16 and need % 16 == 0 and need == int(par.L.par_stft_pan_scratch_bytes(host.ctypes.data, nb))
    Lg, Rg = S.Guarded(par.torch, L.size, L), S.Guarded(par.torch, R.size, R)
    res = []
    for _ in range(2):
        fac, cnt = _outputs(par, nb)
        scratch = S.Guarded(par.torch, need // 4)
        args = (par.dev, Lg.ptr(), Rg.ptr(), frames, bins, 0 if pitch == bins else pitch, ctypes.c_void_p(dev_boxes.data_ptr()),
                host.ctypes.data, nb, fac.ptr(), cnt.ptr(), scratch.ptr())
        if short:
            assert par.L.par_pan_ratio_f32(*args, need - 1, par.stream()) == 4
        par.check(par.L.par_pan_ratio_f32(*args, need, par.stream()))
        res.append(_read(par, fac, cnt, scratch))
    assert Lg.unchanged() and Rg.unchanged()
    assert np.array_equal(res[0][0].view(np.uint64), res[1][0].view(np.uint64)) and np.array_equal(res[0][1], res[1][1]), "two runs differ"
    return res[0]


def check_ratio(par, L, R, bins, cells):
    fac, cnt = run_ratio(par, L, R, bins, cells, short=True)
    for k, cell in enumerate(np.asarray(cells).reshape(-1, 4)):
        want, n, mean_abs = N.box_fsum(L, R, cell)
        assert cnt[k] == n, (k, cell, cnt[k], n)
        if n == 0 or not math.isfinite(want):
            assert (math.isnan(want) and math.isnan(fac[k])) or fac[k] == want, (k, cell, fac[k], want)
        else:
            assert abs(fac[k] - want) <= N.b_ratio(n, mean_abs), (k, cell, fac[k], want, N.b_ratio(n, mean_abs))
    return fac, cnt


def spectra(bins, frames, pitch, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        m = np.full((frames, pitch), S.SENTINEL, dtype=np.float32)
        m[:, :bins] = np.exp(rng.normal(-3.0, 2.0, (frames, bins))).astype(np.float32) + np.float32(1e-7)
        out.append(m)
    return out


# ------------------------------------------------------------------------------------------------ entry 1
@pytest.mark.parametrize("bins,frames,pad", [(9, 11, 0), (513, 13, 0), (513, 13, 31), (8193, 9, 0), (8193, 9, 7)])
def test_ratio_box_shapes(par, bins, frames, pad):
    L, R = spectra(bins, frames, bins + pad, 100 + bins + pad)
    cells = [(3, 4, 2, 3),                          # one cell
             (1, bins - 3, 4, 5),                   # one frame
             (5, 6, 0, frames),                     # one bin
             (1, bins - 3, 0, frames),              # the full clamped band
             (0, bins, 0, frames),                  # everything the spectrogram holds
             (2, 7, 0, 5),                          # crosses the four-frame block of a workgroup by one frame
             (2, 7, 3, 8), (2, 7, 3, 8),            # overlapping, duplicate
             (4, 4, 0, frames), (4, 8, 5, 5), (7, 3, 0, frames), (bins, bins, frames, frames)]      # empty ones
    fac, cnt = check_ratio(par, L, R, bins, cells)
    assert cnt[0] == 1 and cnt[3] == (bins - 4) * frames and fac[6] == fac[7] and np.all(cnt[8:] == 0) and np.all(np.isnan(fac[8:]))
    for single in (cells[3], cells[0], cells[8]):
        f1, c1 = check_ratio(par, L, R, bins, [single])
        k = cells.index(single)
        assert c1[0] == cnt[k] and (f1[0] == fac[k] or (math.isnan(f1[0]) and math.isnan(fac[k])))   # a box does not depend on its neighbours
    check_ratio(par, L, R, bins, cells[:2])


def test_ratio_65_boxes(par):
    bins, frames = 513, 40
    L, R = spectra(bins, frames, bins, 7)
    rng = np.random.default_rng(8)
    cells = []
    for k in range(65):
        bl, f0 = int(rng.integers(0, bins - 1)), int(rng.integers(0, frames - 1))
        cells.append((bl, int(rng.integers(bl, bins + 1)), f0, int(rng.integers(f0, frames + 1))))
    cells[10] = cells[3]
    cells[20] = (5, 5, 0, frames)
    cells[64] = (0, bins, 0, frames)
    fac, cnt = check_ratio(par, L, R, bins, cells)
    assert fac[10] == fac[3] and cnt[20] == 0 and cnt[64] == bins * frames


def test_ratio_nan_and_inf_cells(par):
    bins, frames = 33, 9
    L, R = spectra(bins, frames, bins, 9)
    L[1, 3] = np.nan
    R[2, 4] = np.nan
    L[3, 5] = R[3, 5] = np.nan
    L[5, 10:20] = np.nan                                  # an all-NaN box
    R[6, 10:20] = np.nan
    R[7, 21] = 0.0                                         # +inf
    L[8, 22], R[8, 22] = -1.0, 0.0                         # -inf
    L[0, 30] = R[0, 30] = 0.0                              # 0 / 0: NaN, skipped
    cells = [(0, bins, 0, 5), (10, 20, 5, 7), (20, 23, 7, 8), (20, 23, 8, 9), (20, 23, 7, 9), (30, 31, 0, 1), (0, bins, 0, frames)]
    fac, cnt = check_ratio(par, L, R, bins, cells)
    assert cnt[0] == 5 * bins - 4 and cnt[1] == 0 and math.isnan(fac[1])
    assert fac[2] == math.inf and fac[3] == -math.inf and cnt[4] == 6 and math.isnan(fac[4])      # inf - inf, as numpy
    assert cnt[5] == 0 and math.isnan(fac[5])


# ------------------------------------------------------------------------------------------------ entry 2
def mode1(par, x_ptr, n, stride, n_fft, hop, zp, win):
    bins, nf = n_fft * zp // 2 + 1, S.n_frames_of(n, n_fft, hop)
    out = par.torch.empty((nf, bins), dtype=par.torch.float32, device="cuda")
    par.check(par.L.par_stft_f32(par.dev, x_ptr, n, stride, n_fft, hop, zp, win.ptr(), ctypes.c_void_p(out.data_ptr()), 1, 0, par.stream()))
    return out.cpu().numpy()


def run_fused(par, sig, c_l, c_r, n_fft, hop, zp, cells, layout="interleaved", short=False):
    """sig (n, ch) float32 -> (fac, count, L, R): the fused entry, called twice, and par_stft_f32 mode 1 of the same device samples"""
    n, ch = sig.shape
    win = S.Guarded(par.torch, n_fft, S.window32("blackmanharris", n_fft))
    if layout == "planar":
        bufs = [S.Guarded(par.torch, n, sig[:, c_l].copy()), S.Guarded(par.torch, n, sig[:, c_r].copy())]
        ptrs, stride = [b.ptr() for b in bufs], 1
    else:
        guard = 63 if layout == "odd" else 64           # odd: the pair starts 4 bytes off the 8-byte grid (no paired loads)
        bufs = [S.Guarded(par.torch, n * ch, sig, guard=guard)]
        base = bufs[0].t.data_ptr() + 4 * guard
        ptrs, stride = [ctypes.c_void_p(base + 4 * c_l), ctypes.c_void_p(base + 4 * c_r)], ch
    host, dev_boxes = _boxes(par, cells)
    nb = len(host)
    need = int(par.L.par_stft_pan_scratch_bytes(host.ctypes.data, nb))
    res = []
    for _ in range(2):
        fac, cnt = _outputs(par, nb)
        scratch = S.Guarded(par.torch, need // 4)
        args = (par.dev, ptrs[0], ptrs[1], stride, n, n_fft, hop, zp, win.ptr(), ctypes.c_void_p(dev_boxes.data_ptr()), host.ctypes.data, nb,
                fac.ptr(), cnt.ptr(), scratch.ptr())
        if short:
            assert par.L.par_stft_pan_ratio_f32(*args, need - 1, par.stream()) == 4
        par.check(par.L.par_stft_pan_ratio_f32(*args, need, par.stream()))
        res.append(_read(par, fac, cnt, scratch))
    assert np.array_equal(res[0][0].view(np.uint64), res[1][0].view(np.uint64)) and np.array_equal(res[0][1], res[1][1]), "two runs differ"
    L, R = (mode1(par, p, n, stride, n_fft, hop, zp, win) for p in ptrs)
    assert all(b.unchanged() for b in bufs) and win.unchanged()
    return res[0][0], res[0][1], L, R


def check_fused(par, sig, c_l, c_r, n_fft, hop, zp, cells, layout="interleaved", short=False):
    fac, cnt, L, R = run_fused(par, sig, c_l, c_r, n_fft, hop, zp, cells, layout, short)
    bins = n_fft * zp // 2 + 1
    fac1, cnt1 = run_ratio(par, L, R, bins, cells)
    for k, cell in enumerate(np.asarray(cells).reshape(-1, 4)):
        want, n, mean_abs = N.box_fsum(L, R, cell)
        assert cnt[k] == cnt1[k] == n, (k, cell, cnt[k], cnt1[k], n)
        if n == 0 or not math.isfinite(want):
            assert (math.isnan(fac1[k]) and math.isnan(fac[k])) or fac[k] == fac1[k], (k, cell, fac[k], fac1[k])
        else:
            b = N.b_fused(n, mean_abs)
            print(f"\nfused n_fft={n_fft} zp={zp} hop={hop} {layout} box {tuple(cell)}: |fused - entry 1| = {abs(fac[k] - fac1[k]):.3g}, "
                  f"B_fused {b:.3g}", end="")
            assert abs(fac[k] - fac1[k]) <= b and abs(fac[k] - want) <= b, (k, cell, fac[k], fac1[k], want, b)
    return fac, cnt


def stereo(n, ch, seed, gains=(1.0, 0.6, 0.3, 0.8)):
    rng = np.random.default_rng(seed)
    common = rng.standard_normal(n)
    return np.stack([g * common + 0.3 * rng.standard_normal(n) for g in gains[:ch]], axis=1).astype(np.float32)


def edge_cells(n_fft, zp, hop, n, group):
    """boxes on the first and the last frame (reflected edges), of group - 1, group and group + 1 frames (a workgroup's slots),
    overlapping ones, an empty one and the whole clamped band"""
    bins, nf = n_fft * zp // 2 + 1, S.n_frames_of(n, n_fft, hop)
    hi = max(2, bins - 3)
    cells = [(1, hi, 0, 1), (1, hi, nf - 1, nf), (0, bins, 0, nf), (2, 2, 0, nf), (1, hi, 0, nf)]
    for k in (group - 1, group, group + 1):
        if 0 < k <= nf:
            cells += [(1, min(5, bins), 0, k), (bins // 2, bins, nf - k, nf)]
    return cells


@pytest.mark.parametrize("n_fft,zp,hop,n,group", [
    (16, 1, 4, 1100, 256), (64, 1, 16, 1200, 64), (1024, 1, 256, 3000, 4), (2048, 1, 512, 5000, 2), (16384, 1, 4096, 40000, 1),
    (512, 2, 128, 2000, 4),
    (32, 1, 8, 1025, 128), (128, 1, 32, 1025, 32), (8192, 1, 2048, 2049, 1),     # 2, 8 and 512 lanes per frame: group + 1 frames at hop n_fft / 4
    (256, 1, 256, 3000, 8),            # hop == n_fft
    (64, 1, 1, 200, 64),               # hop == 1
    (1024, 1, 256, 300, 4)])           # a signal shorter than n_fft / 2: every frame reflects, more than once
def test_fused_sizes(par, n_fft, zp, hop, n, group):
    sig = stereo(n, 2, n_fft + zp + hop)
    check_fused(par, sig, 0, 1, n_fft, hop, zp, edge_cells(n_fft, zp, hop, n, group), short=True)


@pytest.mark.parametrize("n_fft,hop,n,group", [(64, 16, 1200, 64), (2048, 512, 5000, 2)])
def test_fused_layouts(par, n_fft, hop, n, group):
    cells = edge_cells(n_fft, 1, hop, n, group)
    sig2, sig4 = stereo(n, 2, 5), stereo(n, 4, 6)
    a, ca = check_fused(par, sig2, 0, 1, n_fft, hop, 1, cells)                        # interleaved pair: 8-byte loads
    b, cb = check_fused(par, sig2, 0, 1, n_fft, hop, 1, cells, "odd")                 # the same pair off the 8-byte grid
    c, cc = check_fused(par, sig2, 0, 1, n_fft, hop, 1, cells, "planar")
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True) and np.array_equal(ca, cb) and np.array_equal(ca, cc)
    check_fused(par, sig4, 0, 1, n_fft, hop, 1, cells)                                # adjacent channels at stride ch + 2
    check_fused(par, sig4, 3, 1, n_fft, hop, 1, cells)                                # right before left
    swapped, _ = check_fused(par, sig2, 1, 0, n_fft, hop, 1, cells[:2])
    assert swapped[0] != a[0]
    same, cs = check_fused(par, sig2, 1, 1, n_fft, hop, 1, cells[:2])
    assert same[0] == 1.0 and same[1] == 1.0


@pytest.mark.parametrize("n_fft,hop,n", [(64, 16, 200), (2048, 512, 5000)])
def test_fused_quotients_are_mode_1s_cell_by_cell(par, n_fft, hop, n):
    """one box per cell of the first, a middle and the last frame: the fused kernel's float32 quotient of every cell is the
    quotient of par_stft_f32's mode-1 magnitudes bit for bit (what NOTES.md states and B_fused rests on)"""
    sig = stereo(n, 2, 21 + n_fft)
    bins, nf = n_fft // 2 + 1, S.n_frames_of(n, n_fft, hop)
    cells = [(b, b + 1, f, f + 1) for f in (0, nf // 2, nf - 1) for b in range(bins)]
    fac, cnt, L, R = run_fused(par, sig, 0, 1, n_fft, hop, 1, cells)
    want = np.concatenate([N.quotients(L[f, :bins], R[f, :bins]) for f in (0, nf // 2, nf - 1)]).astype(np.float64)
    assert np.all(cnt == 1) and np.array_equal(fac, want)


def test_fused_floor_and_nan(par):
    n_fft, hop, n = 1024, 256, 4000
    sig = stereo(n, 2, 11)
    sig[:, 1] *= np.float32(1e-9)                           # a near-silent right channel: its magnitudes sit at the 1e-7 floor
    cells = edge_cells(n_fft, 1, hop, n, 4)
    fac, _ = check_fused(par, sig, 0, 1, n_fft, hop, 1, cells)
    assert fac[2] > 1e4
    sig = stereo(n, 2, 12)
    sig[2000, 0] = np.nan                                   # frames 6 .. 9 of the left channel are NaN throughout
    nf = S.n_frames_of(n, n_fft, hop)
    fac, cnt = check_fused(par, sig, 0, 1, n_fft, hop, 1, [(1, 100, 0, nf), (1, 100, 6, 10), (1, 100, 5, 7)])
    assert cnt[0] == 99 * (nf - 4) and cnt[1] == 0 and math.isnan(fac[1]) and cnt[2] == 99


# ------------------------------------------------------------------------------------------------ entry 3
def run_apply(par, sig, xp, fp, in_stride=1, out_stride=1):
    n = len(sig)
    src = S.Guarded(par.torch, n * in_stride, S.interleave(sig, in_stride))
    xp_t, fp_t = par.torch.from_numpy(np.asarray(xp, dtype=np.float64)).cuda(), par.torch.from_numpy(np.asarray(fp, dtype=np.float64)).cuda()
    res = []
    for _ in range(2):
        out = S.Guarded(par.torch, n * out_stride)
        par.check(par.L.par_pan_apply_f32(par.dev, src.ptr(), in_stride, n, ctypes.c_void_p(xp_t.data_ptr()), ctypes.c_void_p(fp_t.data_ptr()),
                                          len(xp), out.ptr(), out_stride, par.stream()))
        par.torch.cuda.synchronize()
        flat, ok = out.read()
        assert ok and src.unchanged()
        rows = flat.reshape(n, out_stride)
        assert S.is_sentinel(rows[:, 1:]).all(), "cells between the outputs written"
        res.append(rows[:, 0].copy())
    assert np.array_equal(res[0].view(np.uint32), res[1].view(np.uint32))
    return res[0]


def same_floats(got, want):
    """bit for bit where numpy's result is a number; NaN where it is NaN"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


@pytest.mark.parametrize("n,m,in_stride,out_stride", [(1, 1, 1, 1), (1, 2, 1, 1), (777, 1, 1, 1), (777, 2, 2, 3), (5000, 1000, 1, 1),
                                                      (5000, 1000, 3, 2)])
def test_apply_equals_numpy(par, n, m, in_stride, out_stride):
    rng = np.random.default_rng(n + m)
    sig = rng.standard_normal(n).astype(np.float32)
    xp = np.sort(rng.uniform(n * 0.1, n * 0.9, m))          # samples before the first knot and behind the last
    if m >= 4:
        xp[: m // 4] = np.floor(xp[: m // 4])               # knots exactly on samples
        xp.sort()
        xp[m // 2] = xp[m // 2 - 1]                         # a repeated knot
    if n == 1:
        xp = xp * 0.0 + (0.0 if m == 1 else np.array([-1.0, 1.0]))
    fp = rng.standard_normal(m) + 1.0
    assert same_floats(run_apply(par, sig, xp, fp, in_stride, out_stride), N.interp_apply(sig, xp, fp))


def test_apply_nan_and_inf(par):
    n = 400
    rng = np.random.default_rng(3)
    sig = rng.standard_normal(n).astype(np.float32)
    sig[[5, 120, 300]] = [np.nan, np.inf, -np.inf]
    sig[200] = 0.0
    xp = np.array([10.0, 50.0, 50.0, 90.0, 130.5, 170.0, 210.0, 250.0, 290.0, 330.0])
    fp = np.array([1.0, 2.0, np.nan, 1.5, np.inf, 0.5, -np.inf, 1.0, np.nan, 2.0])
    assert same_floats(run_apply(par, sig, xp, fp), N.interp_apply(sig, xp, fp))
    fp2 = np.array([np.inf, np.inf, 1.0, 1.0, -np.inf, -np.inf, 3.0, 3.0, 3.0, np.nan])       # equal infinite neighbours: numpy's retry
    assert same_floats(run_apply(par, sig, xp, fp2), N.interp_apply(sig, xp, fp2))


def test_apply_indices_above_2_to_24(par):
    n = (1 << 24) + 1500
    sig = np.random.default_rng(4).standard_normal(n).astype(np.float32)
    xp = np.array([0.0, 1e7, float(1 << 24) + 0.5, float(1 << 24) + 1001.0, float(n)])
    fp = np.array([1.0, 0.25, 3.0, -2.0, 0.5])
    got = run_apply(par, sig, xp, fp)
    want = N.interp_apply(sig, xp, fp)
    assert same_floats(got, want) and not np.array_equal(want[1 << 24:][:-1], want[1 << 24:][1:])


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("fused", [True, False])
def test_pan_samples_against_the_reference(par, g, tape, fused, monkeypatch):
    from pyaudiorestoration_amd import pypan
    monkeypatch.setattr(pypan, "FUSED", fused)
    sr, fft, overlap, hop = int(g["sr"]), int(g["fft_size"]), int(g["fft_overlap"]), int(g["hop"])
    for zp, boxes, cells, facs in ((1, g["boxes"], g["cells"], g["fac"]), (int(g["zeropad2"]), g["boxes_zp2"], g["cells_zp2"], g["fac_zp2"])):
        got = pypan.pan_samples(tape, sr, [tuple(b) for b in boxes], fft, overlap, zeropad=zp)
        assert len(got) == len(facs)
        for s, box, cell, want in zip(got, boxes, cells, facs):
            assert s.to_cfg()[:4] == tuple(box) and s.t == (box[0] + box[2]) / 2
            if math.isnan(want):
                assert math.isnan(s.pan)
                continue
            b = N.b_ref(tape, 0, 1, fft, hop, zp, cell, want, float(g["s0"]), g["small_L"].size)
            print(f"\npan_samples fused={fused} zp={zp} box {tuple(cell)}: |got - reference| = {abs(s.pan - want):.3g}, B_ref {b:.3g}", end="")
            assert abs(s.pan - want) <= b, (fused, zp, cell, s.pan, want, b)


def test_pan_samples_unsupported_size_takes_the_composed_path(par, tape, monkeypatch):
    from pyaudiorestoration_amd import pypan
    assert pypan.fused_supported(4096, 4) and not pypan.fused_supported(4096, 8) and not pypan.fused_supported(1000)
    # 32768 points: the four-step transform twice, then entry 1 -- against the float64 statement of the same measurement, under
    # B_ref's terms with the four-step kernel's R
    fft, overlap, box = 32768, 8, (0.4, 300.0, 1.0, 4000.0)
    hop, bins, nf = fft // overlap, fft // 2 + 1, S.n_frames_of(len(tape), fft, fft // overlap)
    cell = pypan.box_to_cells(box[:2], box[2:], N.SR, fft, hop, bins, nf)
    bl, bu, f0, f1 = cell
    assert bu > bl and f1 - f0 >= 2
    fr = np.arange(f0, f1)
    want = float(np.mean(N.mags64(tape[:, 0], fft, hop, 1, fr)[:, bl:bu] / N.mags64(tape[:, 1], fft, hop, 1, fr)[:, bl:bu]))
    b = N.b_ref(tape, 0, 1, fft, hop, 1, cell, want, 0.0, 95, r=S.R_FOUR)
    for fused in (True, False):
        monkeypatch.setattr(pypan, "FUSED", fused)
        got = pypan.pan_samples(tape, N.SR, [box], fft, overlap)[0].pan
        print(f"\ncomposed path at {fft} points: |got - float64 statement| = {abs(got - want):.3g}, bound {b:.3g}", end="")
        assert abs(got - want) <= b, (got, want, b)


def test_process_equals_the_references_file(par, g, tape, tmp_path):
    from pyaudiorestoration_amd import io_ops, pypan
    sr, fft, overlap = int(g["sr"]), int(g["fft_size"]), int(g["fft_overlap"])
    wav = str(tmp_path / "tape.wav")
    io_ops.write_wav_float(wav, tape, sr)
    idx, want = g["out_idx"].astype(np.int64), g["out"].astype(np.float32)
    # the fixture's own markers through a .pan project: bit for bit
    project = str(tmp_path / "tape.pan")
    pypan.save_project(project, {"fft_size": fft, "fft_overlap": overlap, "fft_zeropad": 1, "source": wav,
                                 "markers": [tuple(r) for r in g["markers"]]})
    assert sorted(json.load(open(project))) == ["fft_overlap", "fft_size", "fft_zeropad", "markers", "source"]
    written, markers = pypan.process(project=project)
    assert written == str(tmp_path / "tape_out.wav") and len(markers) == len(g["markers"])
    out, sr2, ch = io_ops.read_file(written)
    assert (sr2, ch) == (sr, 1) and out.shape == (len(tape), 1)                      # only the corrected right channel, mono
    assert np.array_equal(out[idx, 0].view(np.uint32), want.view(np.uint32))
    # the extension: the untouched left channel beside it
    written2, _ = pypan.process(wav, project=project, out_suffix="_both", keep_left=True)
    both, _, ch2 = io_ops.read_file(written2)
    assert ch2 == 2 and np.array_equal(both[:, 0], tape[:, 0]) and np.array_equal(both[:, 1], out[:, 0])
    # measured markers: each pan is within B_ref of the reference's, np.interp is a convex combination of them, the product scales
    # that by the sample, and the float32 store rounds once
    finite = [k for k, f in enumerate(g["fac"]) if math.isfinite(f)]
    bmax = max(N.b_ref(tape, 0, 1, fft, fft // overlap, 1, g["cells"][k], g["fac"][k], float(g["s0"]), g["small_L"].size) for k in finite)
    written3, measured = pypan.process(wav, boxes=[tuple(g["boxes"][k]) for k in finite], out_suffix="_measured", fft_size=fft,
                                       fft_overlap=overlap)
    got = io_ops.read_file(written3)[0][idx, 0]
    tol = np.abs(tape[idx, 1]).astype(np.float64) * bmax + 2.0 ** -23 * np.abs(want)
    assert np.all(np.abs(got.astype(np.float64) - want) <= tol), float(np.max(np.abs(got.astype(np.float64) - want) - tol))
    assert [m.to_cfg()[:4] for m in measured] == [tuple(g["boxes"][k]) for k in finite]
    # without markers nothing is written, as in the reference
    assert pypan.process(wav, out_suffix="_none") == (None, []) and not os.path.exists(str(tmp_path / "tape_none.wav"))


def test_cli_pan_round_trip(par, g, tape, tmp_path):
    from pyaudiorestoration_amd import cli, io_ops
    wav, project = str(tmp_path / "t.wav"), str(tmp_path / "t.pan")
    io_ops.write_wav_float(wav, tape, int(g["sr"]))
    box = lambda k: ",".join(repr(float(v)) for v in g["boxes"][k])
    assert cli.main(["pan", "--box", box(0), "--fft", "1024", "--overlap", "4", wav, "--out", project]) == 0
    assert not os.path.exists(str(tmp_path / "t_out.wav"))
    assert cli.main(["pan", "--box", box(4), "--box", box(2), "--fft", "1024", "--overlap", "4", wav, "--out", project]) == 0    # appended
    cfg = json.load(open(project))
    assert len(cfg["markers"]) == 3 and cfg["source"] == wav and cfg["fft_size"] == 1024 and cfg["fft_overlap"] == 4
    for row, k in zip(cfg["markers"], (0, 4, 2)):
        b = N.b_ref(tape, 0, 1, 1024, 256, 1, g["cells"][k], g["fac"][k], float(g["s0"]), g["small_L"].size)
        assert tuple(row[:4]) == tuple(g["boxes"][k]) and abs(row[4] - g["fac"][k]) <= b
    assert cli.main(["pan", project]) == 0
    out, sr, ch = io_ops.read_file(str(tmp_path / "t_out.wav"))
    assert ch == 1 and out.shape == (len(tape), 1) and np.all(np.isfinite(out))
