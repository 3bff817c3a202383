"""par_stft_mean_db_f32 at the C ABI, on the GPU: against math.fsum over 20 log10 of the float32 magnitudes par_stft_f32 mode 1
writes for the same device samples, under the bound of tests/difeq_np.py.  `mean` and `scratch` lie between sentinel cells that
must survive, the scratch is pre-filled with NaN, every call is made twice (bit-identical), channel c of a two-channel call equals
the one-channel call on x + c bit for bit, and channels beyond n_ch hold NaN that must reach no result."""
import ctypes

import numpy as np
import pytest

import difeq_np as D
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


def samples(k):
    """(n, stride) float32: channel c < n_ch holds the case's signal (another seed per channel), the others the sentinel NaN"""
    sig = np.full((k.n, k.stride), S.SENTINEL, dtype=np.float32)
    for c in range(k.n_ch):
        sig[:, c] = np.zeros(k.n, dtype=np.float32) if k.sig == "zero" else S.signal(k.sig, k.n, 7 * k.n_fft + k.n + c)
    return sig


def mode1(par, x_ptr, k, win):
    bins = k.n_fft * k.zp // 2 + 1
    out = par.torch.empty((D.n_frames_of(k.n, k.n_fft, k.hop), bins), dtype=par.torch.float32, device="cuda")
    par.check(par.L.par_stft_f32(par.dev, x_ptr, k.n, k.stride, k.n_fft, k.hop, k.zp, win.ptr(), ctypes.c_void_p(out.data_ptr()), 1, 0,
                                 par.stream()))
    return out.cpu().numpy()


def run_mean(par, x_ptr, k, n_ch, win, short=False):
    """-> mean (n_ch, bins) float64 of one call, made twice on fresh guarded buffers whose scratch holds NaN"""
    bins = k.n_fft * k.zp // 2 + 1
    need = int(par.L.par_stft_mean_db_scratch_bytes(k.n, k.n_fft, k.hop, k.zp, n_ch))
    assert need == D.scratch_bytes(k.n, k.n_fft, k.hop, k.zp, n_ch) and need % 8 == 0
    res = []
    for _ in range(2):
        mean = S.Guarded(par.torch, 2 * n_ch * bins)
        scratch = S.Guarded(par.torch, need // 4, np.full(need // 4, np.nan, dtype=np.float32))
        args = (par.dev, x_ptr, k.n, k.stride, n_ch, k.n_fft, k.hop, k.zp, win.ptr(), mean.ptr(), scratch.ptr())
        if short:
            assert par.L.par_stft_mean_db_f32(*args, need - 1, par.stream()) == 4
        par.check(par.L.par_stft_mean_db_f32(*args, need, par.stream()))
        par.torch.cuda.synchronize()
        m, ok = mean.read()
        assert ok and scratch.read()[1], "guards"
        res.append(m.copy().view(np.float64).reshape(n_ch, bins))
    assert np.array_equal(res[0].view(np.uint64), res[1].view(np.uint64)), "two runs differ"
    return res[0]


@pytest.mark.parametrize("k", D.kernel_cases(), ids=D.case_id)
def test_mean_db_against_fsum_of_mode1(par, k):
    sig = samples(k)
    buf = S.Guarded(par.torch, sig.size, sig)
    win = S.Guarded(par.torch, k.n_fft, S.window32("hann", k.n_fft))
    base = buf.t.data_ptr() + 4 * buf.guard
    mean = run_mean(par, ctypes.c_void_p(base), k, k.n_ch, win, short=(k.n_ch == 2 and k.sig == "noise"))
    assert np.all(np.isfinite(mean)), "a NaN channel or scratch cell reached the result"
    worst = 0.0
    for c in range(k.n_ch):
        mag = mode1(par, ctypes.c_void_p(base + 4 * c), k, win)
        if k.sig == "zero":
            assert np.all(mag == np.float32(1e-7))
        ref, bound = D.mean_db_oracle(mag)
        err = np.abs(mean[c] - ref)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (c, int(np.argmax(err / bound)), float(np.max(err / bound)))
        if k.n_ch > 1:
            one = run_mean(par, ctypes.c_void_p(base + 4 * c), k, 1, win)
            assert np.array_equal(one[0].view(np.uint64), mean[c].view(np.uint64)), f"channel {c} depends on its neighbours"
    print(f"\n{D.case_id(k)}: {D.n_frames_of(k.n, k.n_fft, k.hop)} frames, worst |mean - fsum| / bound {worst:.3f}", end="")
    assert buf.unchanged() and win.unchanged()


@pytest.mark.parametrize("n_fft,hop,zp,n", [(16384, 8192, 1, 8192 * 36 + 5), (4096, 256, 1, 50000), (512, 100, 2, 30001), (16, 3, 1, 2000)])
def test_fused_and_composed_mean_spectra_agree(par, n_fft, hop, zp, n):
    """spectrum_flat.mean_spectra_db_dev: both paths sum the same float32 magnitudes, each within the bound of the fsum oracle"""
    from pyaudiorestoration_amd import fourier, spectrum_flat
    torch = par.torch
    rng = np.random.default_rng(n_fft + hop)
    sig = (rng.standard_normal((n, 3)) * [1.0, 0.01, 0.3]).astype(np.float32)
    sig_t = torch.from_numpy(sig).cuda()
    for channels in ((0, 1, 2), (2, 0), (1,)):
        a = spectrum_flat.mean_spectra_db_dev(sig_t, n_fft, hop, channels, zeropad=zp, fused=True).cpu().numpy()
        b = spectrum_flat.mean_spectra_db_dev(sig_t, n_fft, hop, channels, zeropad=zp, fused=False).cpu().numpy()
        assert a.shape == b.shape == (len(channels), n_fft * zp // 2 + 1) and a.dtype == b.dtype == np.float64
        for i, c in enumerate(channels):
            mag = fourier.stft_dev(sig_t.reshape(-1)[c:], n_fft, hop, fourier.window_dev("hann", n_fft, 0), zp, 1, x_stride=3, n=n, dev=0)
            ref, bound = D.mean_db_oracle(np.ascontiguousarray(mag.T.cpu().numpy()))
            assert np.all(np.abs(a[i] - ref) <= bound) and np.all(np.abs(b[i] - ref) <= bound)
            assert np.all(np.abs(a[i] - b[i]) <= 2 * bound)
    with pytest.raises(ValueError):
        spectrum_flat.mean_spectra_db_dev(sig_t, n_fft, hop, (3,), zeropad=zp)
    # a size the fused kernel does not take goes through the chunked path whatever `fused` says
    big = spectrum_flat.mean_spectra_db_dev(sig_t[:40000], 32768, 16384, (0,), fused=True)
    assert big.shape == (1, 16385) and bool(torch.isfinite(big).all())
