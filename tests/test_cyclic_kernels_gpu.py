"""par_stft_track_peak_f64 and par_cycle_fold_f64 at the C ABI, on the GPU.

The tracker's yardstick is tests/cyclic_np.py applied to the spectrogram par_stft_f32 mode 1 writes for the same device samples:
db = 0 must equal it, and par_track_peak_f64 on that spectrogram, bit for bit in both modes; db = 1 keeps the argmax and stays
within the parabola's bound under one-ulp perturbations of the float32 dB values.  `freqs` lies between sentinel cells, every
call is made twice, unused interleaved channels hold NaN.  The fold equals numpy bit for bit."""
import collections
import ctypes

import numpy as np
import pytest

import cyclic_np as C
import stft_np as S

pytestmark = pytest.mark.gpu
SR = 48000.0


@pytest.fixture(scope="module")
def par():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    from pyaudiorestoration_amd import _dev, _lib

    class P:
        pass
    p = P()
    p.torch, p.dev, p.L, p.check, p.lib, p.stream = torch, 0, _lib.lib(), _lib.check, _lib, lambda: _dev.stream_ptr(0)
    return p


# name, n_fft, zeropad, hop, n, stride, frame_0, count (None: to the last frame), tolerance (octaves), x (float32), trail (per frame
# of the whole file, Hz)
Case = collections.namedtuple("Case", "name n_fft zp hop n stride frame_0 count tol x trail sr")


def frames_per_group(M):
    return S.fft_geom(S.ilog2(M // 2))[2]


def mid_tone(n, M, sr=SR, at=None, noise=1e-4, seed=0):
    """a tone a third of a bin above bin `at` (default M / 4) of the M-point transform, and its frequency"""
    f = ((M // 4 if at is None else at) + 0.3137) * sr / M
    return C.tone(n, sr, f, noise=noise, seed=seed), f


def cases():
    out = []

    def add(name, n_fft, zp, hop, n, stride=1, frame_0=0, count=None, tol=0.31, x=None, trail=None, sr=SR, detune=1.0113):
        M = n_fft * zp
        if x is None:
            x, f = mid_tone(n, M, sr, seed=len(out))
            trail = f * detune if trail is None else trail
        frames = S.n_frames_of(n, n_fft, hop)
        out.append(Case(name, n_fft, zp, hop, n, stride, frame_0, frames - frame_0 if count is None else count, tol, x,
                        np.broadcast_to(np.asarray(trail, dtype=np.float64), (frames,)).copy(), sr))
    # every lane count of a frame (T = 1, 4, 32, 64, 128, 1024), zero-padding 1 / 2 / 4, counts around the frames of a workgroup,
    # a span inside the file
    for n_fft, zp in ((16, 1), (16, 4), (256, 2), (1024, 1), (2048, 1), (4096, 4), (16384, 1)):
        M = n_fft * zp
        F = frames_per_group(M)
        hop = max(1, n_fft // 4)
        n = hop * (F + 4) + 7
        for count, frame_0 in sorted({(1, 0), (max(1, F - 1), 2), (F, 0), (F + 1, 1)}):
            add(f"M{M}_zp{zp}_c{count}_f{frame_0}", n_fft, zp, hop, n, frame_0=frame_0, count=count, tol=0.31 if M > 16 else 0.05)
    # the lane counts between those (T = 2, 8, 16, 512): one frame more than a workgroup holds, both ends reflecting
    for M in (32, 128, 256, 8192):
        add(f"M{M}_group_plus_1", M, 1, M // 4, (M // 4) * frames_per_group(M) + 1)
    add("hop1", 64, 1, 1, 300)
    add("odd_hop", 1024, 1, 341, 9000)
    add("hop_above_n_fft", 256, 2, 300, 3000)
    add("short_1024", 1024, 1, 100, 300)                        # n < n_fft / 2: the reflection repeats
    add("short_16384", 16384, 1, 1000, 5000, sr=22050.0)
    add("stride2", 1024, 1, 256, 3000, stride=2)
    add("stride3_zp4", 4096, 4, 1024, 9000, stride=3)
    add("stride2_T1", 16, 1, 4, 700, stride=2, tol=0.05)
    # 16384 / 128, 313 frames: a glide under a trail that moves with it
    n, sr = 40000, 22050.0
    glide = np.linspace(680.0, 720.0, n)
    frames = S.n_frames_of(n, 16384, 128)
    add("moving_trail", 16384, 1, 128, n, x=C.tone(n, sr, glide, noise=1e-4, seed=3), trail=np.linspace(684.3, 723.1, frames), tol=0.2,
        sr=sr)
    # bands beside the tone: the maximum is the band's first (band above the tone) or last bin (band below), no peak
    x, f = mid_tone(n, 16384, sr, at=520, noise=0.0)
    # (frames whose window lies inside the signal: at the reflected ends the band's edge can be a peak of its own)
    add("first_bin", 16384, 1, 128, n, x=x, trail=(520 + 4.9) * sr / 16384, tol=0.001, sr=sr, frame_0=66, count=180)
    add("last_bin", 16384, 1, 128, n, x=x, trail=(520 - 3.9) * sr / 16384, tol=0.001, sr=sr, frame_0=66, count=180)
    x, f = mid_tone(6000, 1024, at=3, noise=0.0)
    add("NL1", 1024, 1, 256, 6000, x=x, trail=2.6 * SR / 1024, tol=0.9)
    add("bin0", 256, 1, 64, 3000, x=(C.tone(3000, SR, 300.0) + np.float32(0.6)), trail=300.0, tol=0.2 / 12)   # band (0, 4), its peak on bin 0
    add("silence", 1024, 1, 256, 3000, x=np.zeros(3000, dtype=np.float32), trail=5000.0)
    add("silence_16384", 16384, 1, 128, 20000, x=np.zeros(20000, dtype=np.float32), trail=700.0, tol=10 / 12, sr=22050.0)
    return out


CASES = cases()


class Dev:
    """the case's samples (interleaved, NaN in the unused channels), window and mode-1 spectrogram on the device"""

    def __init__(self, par, k):
        self.sig = S.Guarded(par.torch, k.n * k.stride, S.interleave(k.x, k.stride))
        self.win = S.Guarded(par.torch, k.n_fft, S.window32("hann", k.n_fft))
        self.bins = k.n_fft * k.zp // 2 + 1
        self.frames = S.n_frames_of(k.n, k.n_fft, k.hop)
        assert self.frames == par.L.par_stft_frames(k.n, k.n_fft, k.hop)
        self.mag_t = par.torch.empty((self.frames, self.bins), dtype=par.torch.float32, device="cuda")
        par.check(par.L.par_stft_f32(par.dev, self.sig.ptr(), k.n, k.stride, k.n_fft, k.hop, k.zp, self.win.ptr(),
                                     ctypes.c_void_p(self.mag_t.data_ptr()), 1, 0, par.stream()))
        self.mag = self.mag_t.cpu().numpy()


def fused(par, k, d, mode, db, expect=0):
    """-> freqs float64[count] of par_stft_track_peak_f64, called twice on fresh guarded buffers"""
    res = []
    for _ in range(2):
        fr = S.Guarded(par.torch, 2 * k.count, k.trail[k.frame_0:k.frame_0 + k.count].copy().view(np.float32))
        status = par.torch.full((1,), 77, dtype=par.torch.int32, device="cuda")
        rc = par.L.par_stft_track_peak_f64(par.dev, d.sig.ptr(), k.n, k.stride, k.n_fft, k.hop, k.zp, d.win.ptr(), k.frame_0, k.count,
                                           fr.ptr(), k.sr, k.tol, mode, db, ctypes.c_void_p(status.data_ptr()), par.stream())
        assert rc == expect, (rc, par.lib.last_error())
        got, ok = fr.read()
        assert ok, "guards around freqs"
        res.append(got.copy().view(np.float64))
    assert np.array_equal(res[0].view(np.uint64), res[1].view(np.uint64)), "two runs differ"
    assert d.sig.unchanged() and d.win.unchanged()
    return res[0]


def composed(par, k, d, mode):
    f_t = par.torch.from_numpy(k.trail[k.frame_0:k.frame_0 + k.count].copy()).cuda()
    status = par.torch.zeros(1, dtype=par.torch.int32, device="cuda")
    par.check(par.L.par_track_peak_f64(par.dev, ctypes.c_void_p(d.mag_t.data_ptr()), d.frames, d.bins, 0, k.frame_0, k.count,
                                       ctypes.c_void_p(f_t.data_ptr()), k.n_fft * k.zp, k.sr, k.tol, mode, ctypes.c_void_p(status.data_ptr()),
                                       par.stream()))
    return f_t.cpu().numpy()


@pytest.mark.parametrize("k", CASES, ids=[k.name for k in CASES])
def test_db0_equals_the_restatement_and_k_track_bit_for_bit(par, k):
    d = Dev(par, k)
    assert np.all(np.isfinite(d.mag)), "a NaN channel reached the spectrogram"
    trail = k.trail[k.frame_0:k.frame_0 + k.count]
    for mode in (0, 1):
        want, status, seen = C.track(d.mag, k.frame_0, trail, k.n_fft * k.zp, k.sr, k.tol, mode)
        assert status == 0, status
        got = fused(par, k, d, mode, 0)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (mode, int(np.argmax(got != want)), got[got != want][:3], want[got != want][:3])
        assert np.array_equal(got.view(np.uint64), composed(par, k, d, mode).view(np.uint64)), mode
        # what the case is there for
        bins_hit = np.array([a for _, _, a in seen])
        on_bin = want == bins_hit / (k.n_fft * k.zp) * k.sr
        if k.name in ("first_bin", "last_bin"):
            edge = np.array([NL if k.name == "first_bin" else NU - 1 for NL, NU, _ in seen])
            assert np.array_equal(bins_hit, edge) and np.all(on_bin)
        elif k.name == "NL1":
            assert all(NL == 1 for NL, _, _ in seen) and not np.any(on_bin)
        elif k.name == "bin0":
            assert seen[0][:2] == (0, 4) and 0 in bins_hit
        elif k.name.startswith("silence"):
            assert np.all(d.mag == np.float32(1e-7)) and np.array_equal(bins_hit, [NL for NL, _, _ in seen]) and np.all(on_bin)
        elif k.name == "moving_trail":
            assert len({(NL, NU) for NL, NU, _ in seen}) >= (3 if mode == 0 else 2) and not np.any(on_bin)
        elif k.name.startswith("short"):
            assert k.n < k.n_fft // 2


DB_CASES = [k for k in CASES if k.name in ("M16384_zp1_c1_f0", "M16384_zp4_c2_f1", "M2048_zp1_c3_f1", "M1024_zp1_c5_f1", "M512_zp2_c9_f1",
                                            "M64_zp4_c65_f1", "odd_hop", "stride3_zp4", "moving_trail", "short_16384", "NL1")]
assert len(DB_CASES) == 11


@pytest.mark.parametrize("k", DB_CASES, ids=[k.name for k in DB_CASES])
def test_db1_keeps_the_argmax_and_stays_within_the_parabola_bound(par, k):
    d = Dev(par, k)
    db = C.to_db32(d.mag)
    trail = k.trail[k.frame_0:k.frame_0 + k.count]
    worst = 0.0
    for mode in (0, 1):
        want, status, seen = C.track(db, k.frame_0, trail, k.n_fft * k.zp, k.sr, k.tol, mode)
        assert status == 0
        bound = np.empty(k.count)
        for i, (NL, NU, arg) in enumerate(seen):
            row = db[k.frame_0 + i]
            rest = np.delete(row[NL:NU], arg - NL)
            assert row[arg] - 2 * np.spacing(row[arg]) > rest.max(), "the band maximum must beat the others by more than 2 ulps"
            assert row[arg - 1] < row[arg] > row[arg + 1]
            bound[i] = C.parabola_bound(row, arg, k.n_fft * k.zp, k.sr)
        got = fused(par, k, d, mode, 1)
        assert np.array_equal(np.rint(got * (k.n_fft * k.zp) / k.sr), [a for _, _, a in seen]), "argmax"
        err = np.abs(got - want)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (mode, int(np.argmax(err / bound)), float(np.max(err / bound)))
    print(f"\n{k.name}: worst |freq - restatement| / bound {worst:.3g}", end="")


def test_status_paths_are_error_returns_of_valid_launches(par):
    """a trail below the transform's resolution, a peak on the last bin, a band past the last bin"""
    from pyaudiorestoration_amd import cyclic_wow as W
    n, M = 3000, 64
    nyq = np.tile(np.array([0.5, -0.5], dtype=np.float32), n // 2)
    bins = M // 2 + 1
    f_last, tol_last = 31 * SR / M, 0.03
    assert C.band_limits(1.0, 0.3, 1024, SR, 513) == (-1, 3, False)
    assert C.band_limits(f_last, tol_last, M, SR, bins) == (bins - 4, bins, False)
    assert C.band_limits(SR / 2 * 0.9999, 1e-4, M, SR, bins) == (bins - 3, bins, True)
    for name, (n_fft, x, freq, tol, code, exc) in {
            "empty": (1024, mid_tone(n, 1024)[0], 1.0, 0.3, 5, ValueError),
            "last_bin": (M, nyq, f_last, tol_last, 6, IndexError),
            "past_end": (M, nyq, SR / 2 * 0.9999, 1e-4, 7, ValueError)}.items():
        k = Case(name, n_fft, 1, n_fft // 4, n, 1, 1, 9, tol, x, np.full(S.n_frames_of(n, n_fft, n_fft // 4), freq), SR)
        d = Dev(par, k)
        for mode in (0, 1):
            got = fused(par, k, d, mode, 0, expect=code)
            want, status, _ = C.track(d.mag, 1, k.trail[1:10], n_fft, SR, tol, mode)
            assert status == {5: 1, 6: 2, 7: 4}[code]
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64))        # empty: the trail is left; the others: the integer bin
            assert par.L.par_track_peak_f64(par.dev, ctypes.c_void_p(d.mag_t.data_ptr()), d.frames, d.bins, 0, 1, 9,
                                            ctypes.c_void_p(par.torch.from_numpy(k.trail[1:10].copy()).cuda().data_ptr()), n_fft, SR, tol,
                                            mode, ctypes.c_void_p(par.torch.zeros(1, dtype=par.torch.int32, device="cuda").data_ptr()),
                                            par.stream()) == code
        for fused_path in (True, False):
            with pytest.raises(exc) as e:
                W.pilot_track(x, SR, [(0.0, freq), (n / SR, freq)], n_fft, n_fft // 4, tol * 12, db=False, fused=fused_path)
            assert isinstance(e.value, par.lib.ParError) and e.value.code == code
    # the launch after an error return is a clean one
    k = CASES[0]
    fused(par, k, Dev(par, k), 0, 0)


# ---------------------------------------------------------------------------------------------------------------- fold
def run_fold(par, v, p_first, n_cand, with_avg=True, extra_pitch=0):
    """-> (avg rows [list of float64 arrays] or None, delta float64[n_cand]); avg and delta between sentinels, run twice"""
    torch = par.torch
    v_t = torch.from_numpy(np.asarray(v, dtype=np.float64)).cuda()
    pitch = p_first + n_cand - 1 + extra_pitch
    res = []
    for _ in range(2):
        avg = S.Guarded(torch, 2 * n_cand * pitch)
        delta = S.Guarded(torch, 2 * n_cand)
        par.check(par.L.par_cycle_fold_f64(par.dev, ctypes.c_void_p(v_t.data_ptr()), len(v), p_first, n_cand, avg.ptr() if with_avg else None,
                                           pitch, delta.ptr(), par.stream()))
        torch.cuda.synchronize()
        a, ok_a = avg.read()
        dl, ok_d = delta.read()
        assert ok_a and ok_d, "guards"
        a = a.copy().reshape(n_cand, 2 * pitch)
        rows = []
        for c in range(n_cand):
            P = p_first + c
            if with_avg:
                assert np.all(S.is_sentinel(a[c, 2 * P:])), f"row {c}: cells behind the cycle were written"
                rows.append(a[c, :2 * P].copy().view(np.float64))
            else:
                assert np.all(S.is_sentinel(a[c])), "avg = NULL, yet something was written"
        res.append((rows, dl.copy().view(np.float64)))
    assert np.array_equal(res[0][1].view(np.uint64), res[1][1].view(np.uint64))
    assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(res[0][0], res[1][0]))
    assert np.array_equal(v_t.cpu().numpy().view(np.uint64), np.asarray(v, dtype=np.float64).view(np.uint64))
    return (res[0][0] if with_avg else None), res[0][1]


def check_fold(v, p_first, rows, delta):
    for c, d in enumerate(delta):
        P = p_first + c
        want = C.fold_ordered(v, P)
        if P >= 2:
            assert np.array_equal(C.fold(v, P).view(np.uint64), want.view(np.uint64))          # numpy's own order
        if rows is not None:
            assert np.array_equal(rows[c].view(np.uint64), want.view(np.uint64)), (P, len(v))
        dw = np.max(want) - np.min(want)
        assert d == dw or (np.isnan(d) and np.isnan(dw)), (P, d, dw)


V1000 = np.log2(700.0 * (1 + 0.005 * np.sin(np.arange(1000) / 7.0))) + 1e-6 * np.random.default_rng(5).standard_normal(1000)


@pytest.mark.parametrize("p_first,n_cand", [(1, 90), (91, 90), (424, 90)])
def test_fold_ninety_candidates_equal_numpy_bit_for_bit(par, p_first, n_cand):
    rows, delta = run_fold(par, V1000, p_first, n_cand, extra_pitch=3)
    check_fold(V1000, p_first, rows, delta)
    _, delta2 = run_fold(par, V1000, p_first, n_cand, with_avg=False)
    assert np.array_equal(delta.view(np.uint64), delta2.view(np.uint64))


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 255, 256, 257, 512, 513])
def test_fold_single_candidate_at_every_count(par, P):
    for count in sorted({P, 2 * P - 1, 2 * P, 1000}):
        if count < P:
            continue
        v = np.resize(V1000, count) + np.arange(count) * 1e-9
        rows, delta = run_fold(par, v, P, 1)
        check_fold(v, P, rows, delta)
    if P == 1:                                              # numpy sums the single column pairwise: bounded, not equal
        rows, _ = run_fold(par, V1000, 1, 1)
        assert abs(rows[0][0] - C.fold(V1000, 1)[0]) <= C.fold_bound_p1(V1000)


def test_fold_propagates_nan_as_numpy_does(par):
    v = V1000.copy()
    v[300] = np.nan
    rows, delta = run_fold(par, v, 5, 6, extra_pitch=1)
    for c in range(6):
        P = 5 + c
        want = C.fold(v, P)
        assert np.array_equal(np.isnan(rows[c]), np.isnan(want)) and np.isnan(want).sum() == (1 if 300 < 1000 // P * P else 0)
        assert np.array_equal(rows[c][~np.isnan(want)].view(np.uint64), want[~np.isnan(want)].view(np.uint64))
        assert np.isnan(delta[c]) == np.isnan(np.max(want) - np.min(want))
        if not np.isnan(delta[c]):
            assert delta[c] == np.max(want) - np.min(want)
    assert np.isnan(delta).sum() >= 5
