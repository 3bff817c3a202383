"""Host-side checks of the renoiser's offset gauge (K_gauge, renoiser.sniff_offset): the FIR identity the kernel rests on, the
float32 summation order inside the derived bound on every shape the GPU tests use, the band arithmetic against the reference's
numbers, the frame count, the argument errors of the C entry points, and the command line."""
import ctypes

import numpy as np
import pytest

import gauge_np as G
from pyaudiorestoration_amd import _lib, cli, renoiser


def _h32(n_fft, sr=G.SR):
    h = renoiser.gauge_filter(sr, n_fft, G.BAND)
    return h, h.real.astype(np.float32), h.imag.astype(np.float32)


@pytest.mark.parametrize("n_fft,hop,n", [(64, 8, 1000), (64, 16, 777), (256, 32, 5000), (32, 32, 300)])
def test_literal_loop_equals_the_fir_form(n_fft, hop, n):
    x = G.noise_and_tone(n, seed=n)
    ref = G.reference_stds(x, G.SR, n_fft, hop)
    fir = G.fir_stds(x, renoiser.gauge_filter(G.SR, n_fft, G.BAND), n_fft, hop)
    assert ref.shape == fir.shape == (hop,) and np.all(np.isfinite(ref))
    assert np.max(np.abs(ref - fir)) <= 1e-12 * np.max(np.abs(ref))


def _signals(name, n):
    if name == "impulse":
        return [G.impulse(n, 0), G.impulse(n, n - 1), G.impulse(n, n // 2)]
    if name == "tone":
        return [G.tone(n)]
    return [G.noise(n), G.noise_and_tone(n)]


CASES = dict(G.GPU_SHAPES, impulse=G.IMPULSE_SHAPE, tone=G.TONE_SHAPE)


@pytest.mark.parametrize("name", list(CASES))
def test_float32_summation_order_stays_inside_the_bound(name):
    n_fft, hop, n = CASES[name]
    h, hr, hi = _h32(n_fft)
    assert G.sum_constant(n_fft) <= n_fft + 3
    for x in _signals(name, n):
        ref = G.reference_stds(x, G.SR, n_fft, hop)
        emu = G.emulate_f32(x, hr, hi, n_fft, hop)
        tol = G.bound(x, hr + 1j * hi.astype(np.float64), n_fft, hop)
        err = np.abs(emu - ref)
        print(name, "max err", err.max(), "min bound", tol.min(), "max err / bound", (err / tol).max())
        assert np.all(np.isfinite(emu)) and np.all(emu >= 0) and np.all(tol > 0)
        assert np.all(err <= tol)


def test_impulse_shape_puts_a_last_frame_on_the_reflected_last_sample():
    n_fft, hop, n = G.IMPULSE_SHAPE
    hit = [i for i in range(hop) if (n + i + n_fft // 2) % hop == 0]
    assert hit
    i = hit[0]
    p = G.padded(G.impulse(n, n - 1), i, n_fft)
    last = G.frames_of(p, n_fft, hop)[-1]
    assert last[-1] == 1.0 and np.count_nonzero(last) == 1          # the right reflection's very last sample is x[n - 1]
    p0 = G.padded(G.impulse(n, 1), 0, n_fft)
    assert p0[n_fft // 2 - 1] == 1.0 and p0[n_fft // 2 + 1] == 1.0   # the left reflection mirrors real samples


def test_gauge_band_matches_the_reference_numbers():
    assert renoiser.gauge_band(44100, 2048) == (139, 557)
    assert renoiser.gauge_band(44100, 64) == (4, 17)
    assert renoiser.gauge_band(16000, 2048) == (384, 1025)           # u clipped to the number of bins
    with pytest.raises(ValueError, match="no bin"):
        renoiser.gauge_band(4000, 2048)
    for sr, n_fft in ((44100, 2048), (44100, 64), (16000, 2048), (48000, 50)):
        assert renoiser.gauge_band(sr, n_fft, G.BAND) == G.band_bins(sr, n_fft)
    h = renoiser.gauge_filter(44100, 64)
    assert h.dtype == np.complex128 and h.shape == (64,)


def test_gauge_frames_formula():
    L = _lib.lib()
    for n, n_fft, hop in [(50, 16, 4), (1000, 64, 8), (333, 50, 7), (100, 256, 32), (10_584_000, 2048, 512), (1, 2, 1)]:
        for off in sorted({0, 1, hop // 2, hop - 1}):
            want = (n + off + n_fft // 2) // hop + 1
            assert L.par_gauge_frames(n, n_fft, hop, off) == want
            if n <= 2000:                                            # ... which is the reference's own count
                assert want == len(G.frames_of(G.padded(np.zeros(n), off, n_fft), n_fft, hop))
    assert L.par_gauge_frames(-1, 16, 4, 0) == -1 and L.par_gauge_frames(10, 1, 4, 0) == -1
    assert L.par_gauge_frames(10, 16, 0, 0) == -1 and L.par_gauge_frames(10, 16, 4, -1) == -1


def test_argument_errors_come_before_any_device_call():
    L = _lib.lib()
    p = ctypes.c_void_p(64)
    need = L.par_gauge_scratch_bytes(1000, 64, 8)
    assert need > 0 and L.par_gauge_scratch_bytes(0, 64, 8) == 0 and L.par_gauge_scratch_bytes(10, 1, 8) == 0
    assert L.par_gauge_scratch_bytes(10, 64, 0) == 0
    # 4 minutes at 44.1 kHz: three float64 per workgroup and slot, well under the signal's own size at the GUI default
    assert L.par_gauge_scratch_bytes(10_584_000, 2048, 128) < 4 * 10_584_000 * 2

    def call(x=p, n=1000, xs=1, n_fft=64, hop=8, hr=p, hi=p, stds=p, scratch=p, nbytes=need):
        return L.par_gauge_offset_f32(0, x, n, xs, n_fft, hop, hr, hi, stds, scratch, nbytes, None)
    for kw, word in ((dict(x=None), "null x"), (dict(hr=None), "h_re"), (dict(hi=None), "h_im"), (dict(stds=None), "stds"),
                     (dict(scratch=None), "scratch"), (dict(n=0), "n 0"), (dict(n_fft=1), "n_fft"), (dict(hop=0), "hop"),
                     (dict(xs=0), "x_stride"), (dict(nbytes=need - 1), "scratch_bytes")):
        assert call(**kw) == 1, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())


def test_python_entry_points_have_no_cpu_fallback_and_check_offsets_first():
    import torch
    x = G.noise(4000).reshape(-1, 2)
    final = np.full(129, -30.0)
    for bad in (64, -1, 1000):                                       # before any device work: also without a GPU
        with pytest.raises(ValueError, match="offset"):
            renoiser.renoise_offset(x, G.SR, final, bad, 12.0, 256, 64)
        with pytest.raises(ValueError, match="offset"):
            renoiser.renoise_dev(x, final, 12.0, 256, 64, offset=bad)
        with pytest.raises(ValueError, match="offset"):
            renoiser.renoise_file("missing.wav", fft_size=256, overlap=4, offset=bad)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            renoiser.sniff_offset(x, G.SR, 256, 64)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            renoiser.renoise_offset(x, G.SR, final, 3, 12.0, 256, 64)


def test_cli_knows_gauge_and_offset():
    p = cli.parser()
    a = p.parse_args(["renoise", "--gauge", "a.wav"])
    assert a.gauge is True and a.offset == 0
    assert p.parse_args(["renoise", "a.wav"]).gauge is False
    assert p.parse_args(["renoise", "--offset", "17", "a.wav"]).offset == 17
    assert p.parse_args(["renoise", "--offset", "auto", "a.wav"]).offset == "auto"
    with pytest.raises(SystemExit):
        p.parse_args(["renoise", "--offset", "soon", "a.wav"])
