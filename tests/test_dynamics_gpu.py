"""The dynamics matcher's kernels (csrc/dynamics.hip) at the C ABI against the oracles and bounds of tests/dynamics_np.py, and
decompressor.match_dynamics / process / windowed_rms end to end against the reference's stored output.

Every output buffer lies between sentinel cells that must survive; every case runs twice and must repeat bit for bit.
pytest -s prints the measured figures (NOTES.md, Dynamics matcher)."""
import numpy as np
import pytest
import scipy.ndimage

import dynamics_np as D
from test_heal_kernels_gpu import Guarded, bits

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5


@pytest.fixture(scope="module")
def par():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pyaudiorestoration_amd import _dev, _lib

    class P:
        pass
    p = P()
    p.torch, p.dev, p.L, p.check, p.stream = torch, 0, _lib.lib(), _lib.check, lambda: _dev.stream_ptr(0)
    return p


def twice(par, shape, call, dtype=np.float64, fill=SENTINEL):
    """run `call(out_ptr)` into two fresh guarded buffers -> the result (sentinels checked, the two runs equal bit for bit)"""
    got = []
    for _ in range(2):
        out = Guarded(par, np.full(shape, fill, dtype=dtype), 2, fill)
        par.check(call(out.ptr()))
        par.torch.cuda.synchronize()
        got.append(out.read().copy())
        assert out.guards_intact()
    assert np.array_equal(bits(got[0]), bits(got[1]))
    return got[0]


# ------------------------------------------------------------------------------------------ K_wrms
def wrms(par, x, n, hop, sz, floor=D.FLOOR, log10=1):
    """x: (rows, pitch) float64, n samples of each row used"""
    src = Guarded(par, x, 1, 1e300)
    F = D.n_frames(n, hop)
    got = twice(par, (x.shape[0], F), lambda o: par.L.par_windowed_rms_log10_f64(par.dev, src.ptr(), x.shape[1], x.shape[0], n, hop, sz, floor,
                                                                                  log10, o, par.stream()))
    assert src.unchanged()
    return got


def check_wrms_row(got, x, hop, sz, label):
    """one row against the exact-sum oracle under dynamics_np.rms_log_bound; frames within the bound of the floor may sit on
    either side of the clip"""
    want, r = D.log_curve_exact(x, hop, sz)
    bound = D.rms_log_bound(want, sz)
    err = np.abs(got - want)
    near = D.near_floor(r, sz)
    ok = (err <= bound) | (near & (np.abs(got - np.log10(D.FLOOR)) <= bound))
    print(f"\nK_wrms {label}: worst error {float(np.max(err / bound)):.3f} of the bound, {int(near.sum())} frames at the floor's edge")
    assert np.all(ok), (label, np.flatnonzero(~ok)[:5].tolist(), err[~ok][:5], bound[~ok][:5])


# the last three: hops that are no power of two (a lane walks a piece in several steps; 300: all 64 lanes of a wave on a piece)
@pytest.mark.parametrize("n,hop,sz", [(301, 4, 10), (4099, 4, 10), (301, 8, 8), (4099, 8, 8), (301, 16, 5), (4099, 16, 5), (301, 4, 400),
                                      (301, 32, 512), (4099, 32, 512), (301, 6, 10), (4099, 12, 40), (4099, 300, 700)])
def test_windowed_rms_log10(par, n, hop, sz):
    pitch = n + 5                                                        # even (n is odd): rows start on 16 bytes, the 16-byte loads
    x = np.full((3, pitch), 1e300)
    x[0, :n], x[1, :n], x[2, :n] = D.rms_row(n), D.floor_row(n, hop, sz), 0.0
    got = wrms(par, x, n, hop, sz)
    check_wrms_row(got[0], x[0, :n], hop, sz, f"n={n} hop={hop} sz={sz} noise")
    check_wrms_row(got[1], x[1, :n], hop, sz, f"n={n} hop={hop} sz={sz} floor")
    assert np.all(got[2] == np.log10(D.FLOOR))                           # an all-zero row: log10(floor) exactly
    if hop % 2 == 0:                                                     # an odd pitch: the 8-byte loads on the same rows
        x2 = np.full((3, pitch + 1), 1e300)
        x2[:, :n] = x[:, :n]
        got2 = wrms(par, x2, n, hop, sz)
        check_wrms_row(got2[0], x[0, :n], hop, sz, f"n={n} hop={hop} sz={sz} noise, odd pitch")
        assert np.all(got2[2] == np.log10(D.FLOOR))


@pytest.mark.parametrize("n,hop,sz", [(301, 4, 10), (4099, 32, 512), (301, 16, 5)])
def test_windowed_rms_one_nan(par, n, hop, sz):
    """exactly the frames whose window contains the NaN are NaN"""
    x = D.rms_row(n)[None, :].copy()
    at = n // 2 + 1
    x[0, at] = np.nan
    got = wrms(par, x, n, hop, sz)[0]
    starts = np.arange(0, n, hop)
    holds = (starts <= at) & (at < starts + sz)
    assert holds.any() or sz < hop
    assert np.array_equal(np.isnan(got), holds)


# ------------------------------------------------------------------------------------------ K_level
@pytest.mark.parametrize("rows", [1, 4])
@pytest.mark.parametrize("F", [1, 75, 4097])
def test_level_match(par, rows, F):
    a, b = D.level_rows(rows, F)
    ga, gb = Guarded(par, a, 1, 1e300), Guarded(par, b, 1, 1e300)
    got = twice(par, (rows, F), lambda o: par.L.par_level_match_f64(par.dev, ga.ptr(), gb.ptr(), rows, F, o, par.stream()))
    worst = 0.0
    for r in range(rows):
        want = D.level_match_exact(a[r], b[r])
        bound = D.level_bound(a[r], b[r], want)
        err = np.abs(got[r] - want)
        assert np.all(err <= bound), (rows, F, r, err.max(), bound.min())
        worst = max(worst, float(np.max(err / bound)))
    print(f"\nK_level rows={rows} F={F}: worst error {worst:.3f} of the bound")
    assert ga.unchanged() and gb.unchanged()


# ------------------------------------------------------------------------------------------ K_box (reflect)
@pytest.mark.parametrize("n,size", [(75, 6), (75, 7), (75, 1), (5, 12), (1, 4), (6250, 110)])
def test_uniform_filter_reflect(par, n, size):
    x = np.stack((D.box_row(n), D.box_row(n, seed=8)))
    src = Guarded(par, x, 1, 1e300)
    got = twice(par, (2, n), lambda o: par.L.par_uniform_filter_reflect_f64(par.dev, src.ptr(), 2, n, size, o, par.stream()))
    for r in range(2):
        want, peak = D.uniform_reflect_exact(x[r], size)
        err = np.abs(got[r] - want)
        assert np.all(err <= D.box_bound(peak)), (n, size, r, err.max())
        assert np.max(np.abs(got[r] - scipy.ndimage.uniform_filter1d(x[r], size=size))) <= 1e-13
        print(f"\nK_box n={n} size={size} row {r}: worst error {float(np.max(err / D.box_bound(peak))):.3f} of the bound")
    if size == 1:
        assert np.array_equal(bits(got), bits(x))
    assert src.unchanged()


# ------------------------------------------------------------------------------------------ K_dynfac
@pytest.mark.parametrize("corr_sz,F", [(16, 8), (16, 9), (16, 24), (16, 25), (16, 75), (4096, 6250)])
def test_dynamics_factor(par, corr_sz, F):
    rows = 2
    ab = [D.fac_rows(F, corr_sz, seed=9 + r) for r in range(rows)]
    a, b = np.stack([v[0] for v in ab]), np.stack([v[1] for v in ab])
    ga, gb = Guarded(par, a, 1, 1e300), Guarded(par, b, 1, 1e300)
    hann = Guarded(par, np.hanning(corr_sz), 1, 1e300)
    al_buf = Guarded(par, np.full((rows, F), SENTINEL), 2, SENTINEL)
    fac = twice(par, (rows, F), lambda o: par.L.par_dynamics_factor_f64(par.dev, ga.ptr(), gb.ptr(), rows, F, hann.ptr(), corr_sz, al_buf.ptr(),
                                                                        o, par.stream()))
    al = al_buf.read().copy()
    assert al_buf.guards_intact()
    fac_only = twice(par, (rows, F), lambda o: par.L.par_dynamics_factor_f64(par.dev, ga.ptr(), gb.ptr(), rows, F, hann.ptr(), corr_sz, None, o,
                                                                             par.stream()))
    assert np.array_equal(bits(fac_only), bits(fac))                    # the optional output changes nothing
    worst, ch = 0.0, corr_sz // 2
    x_last = ch * ((F - 1) // ch)
    for r in range(rows):
        assert np.array_equal(bits(al[r]), bits(D.aligned_np(a[r], corr_sz))), (corr_sz, F, r)
        want, hard = D.fac_exact(b[r], al[r])
        assert np.array_equal(fac[r][hard], want[hard])
        soft = ~hard
        rel = np.abs(fac[r][soft] - want[soft]) / want[soft]
        assert np.all(rel <= D.FAC_REL), (corr_sz, F, r, rel.max())
        if soft.any():
            worst = max(worst, float(rel.max() / D.U))
        assert fac[r][F // 3] == 0.0                                     # the NaN in b
        assert np.all(al[r][max(x_last - 1, 0):] == 0)                   # the reference's zeroed tail
        if F >= 24:
            assert np.any(fac[r] == 2.0) and np.any((fac[r] > 0) & (fac[r] < 2.0))
    print(f"\nK_dynfac corr_sz={corr_sz} F={F}: worst fac error {worst:.2f} units of 2^-53 relative (bound 64)")
    assert ga.unchanged() and gb.unchanged() and hann.unchanged()


# ------------------------------------------------------------------------------------------ K_dynapply
@pytest.mark.parametrize("n_ch", [1, 2, 3])
@pytest.mark.parametrize("hop,F,full", [(32, 70, False), (32, 70, True), (1, 300, True), (5, 1000, False), (3000, 3, True)])
def test_dynamics_apply(par, n_ch, hop, F, full):
    n = F * hop if full else (F - 1) * hop + 1
    sig, fac = D.apply_case(n, n_ch, hop)
    want = D.apply_np(sig, fac, hop).astype(np.float32)
    gf = Guarded(par, fac, 1, 1e300)
    for pad in (0, 2):                                                   # packed rows (the float2 path for stereo) and wider strides
        body = np.full((n, n_ch + pad), np.float32(7e37), dtype=np.float32)
        body[:, :n_ch] = sig
        s = Guarded(par, body, 4, np.float32(7e37))
        got = twice(par, (n, n_ch + pad), lambda o: par.L.par_dynamics_apply_f32(par.dev, s.ptr(), n_ch + pad, n_ch, n, gf.ptr(), F, hop, o,
                                                                                 n_ch + pad, par.stream()), np.float32, np.float32(-7.25))
        assert np.array_equal(bits(got[:, :n_ch]), bits(want)), (n_ch, hop, F, full, pad)
        assert np.all(got[:, n_ch:] == np.float32(-7.25))                # the cells between the channels stay
        assert s.unchanged()
    assert gf.unchanged()


# ------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def golden_pair():
    g = np.load(D.GOLDEN)
    src, ref = D.golden_input(g)
    return g, src, ref


def check_golden(g, got):
    want = g["out"].astype(np.float32)
    rows = D.golden_rows(len(got))
    err = np.abs(want.astype(np.float64) - got[rows].astype(np.float64))
    tol = 1e-6 * np.max(np.abs(want))
    print(f"\nmatch_dynamics against the reference: worst error {err.max():.3e} ({err.max() / np.max(np.abs(want)):.3e} of the peak), "
          f"{int(np.sum(bits(want) == bits(got[rows])))} of {want.size} samples equal bit for bit")
    assert got.dtype == np.float32 and np.all(err <= tol), (err.max(), tol)


def test_match_dynamics_against_the_reference(par, golden_pair):
    from pyaudiorestoration_amd import decompressor as P
    g, src, ref = golden_pair
    got = P.match_dynamics(src, ref, int(g["sr"]))
    assert isinstance(got, np.ndarray) and got.shape == src.shape
    check_golden(g, got)
    t = P.match_dynamics(par.torch.from_numpy(src).cuda(), par.torch.from_numpy(ref).cuda(), int(g["sr"]))
    assert par.torch.is_tensor(t) and t.is_cuda and t.dtype == par.torch.float32
    assert np.array_equal(bits(t.cpu().numpy()), bits(got))              # device in == numpy in, and two runs repeat
    # a longer ref is truncated to src (and the other way round)
    longer = np.concatenate((ref, ref[:100]))
    assert np.array_equal(bits(P.match_dynamics(src, longer, int(g["sr"]))), bits(got))
    fac = P.gain_curves(src, ref, int(g["sr"]))
    assert fac.shape == (2, D.n_frames(len(src), D.HOP)) and fac.dtype == np.float64 and fac.max() == 2.0 and fac.min() >= 0.0


def test_process_writes_the_references_file(par, golden_pair, tmp_path):
    from pyaudiorestoration_amd import decompressor as P, io_ops
    g, src, ref = golden_pair
    a, b = str(tmp_path / "side a.wav"), str(tmp_path / "side a ref.wav")
    io_ops.write_wav_float(a, src, int(g["sr"]))
    io_ops.write_wav_float(b, ref, int(g["sr"]))
    path = P.process(a, b)
    assert path == a + "decompressed.wav"
    y, sr, ch = io_ops.read_file(path)
    assert sr == int(g["sr"]) and ch == 2 and np.array_equal(bits(y), bits(P.match_dynamics(src, ref, sr)))
    check_golden(g, y)


def test_windowed_rms_is_the_references_loop(par):
    from pyaudiorestoration_amd import decompressor as P
    x = D.floor_row(4099, 32, 512)
    want = D.windowed_rms_np(x, 32, 512)
    got = P.windowed_rms(x, 32, 512)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want.shape
    # relative: gamma_k / 2 + 2 u (dynamics_np.rms_log_bound before the logarithm) for either summation order
    tol = 2 * (D.gamma(513) / 2 + 2 * D.U) * want
    assert np.all(np.abs(got - want) <= tol)
    assert np.any(want == 0) and np.array_equal(got == 0, want == 0)     # silent windows: exactly 0, no floor
    t = P.windowed_rms(par.torch.from_numpy(x).cuda(), 32, 512)
    assert par.torch.is_tensor(t) and np.array_equal(bits(t.cpu().numpy()), bits(got))
