"""K_gauge (par_gauge_offset_f32) and renoiser.sniff_offset on the device against the reference's loop in float64
(tests/gauge_np.py).  The tolerance of every curve comparison is gauge_np.bound: derived from the kernel's summation order, not
tuned.  renoise_offset(..., k) and renoise_dev(..., offset=k) against the padded call, bit for bit."""
import numpy as np
import pytest
import torch

import gauge_np as G
from pyaudiorestoration_amd import _dev, renoiser

pytestmark = pytest.mark.gpu

_cache = {}


def _case(name, x_fn, n_fft, hop, n):
    """(x, float64 reference curve, bound), computed once; the curve and the bound are kept read-only"""
    key = (name, n_fft, hop, n)
    if key not in _cache:
        x = x_fn(n)
        h = renoiser.gauge_filter(G.SR, n_fft, G.BAND)
        h32 = h.real.astype(np.float32) + 1j * h.imag.astype(np.float32).astype(np.float64)
        ref = G.reference_stds(x, G.SR, n_fft, hop)
        tol = G.bound(x, h32, n_fft, hop)
        for a in (ref, tol):
            a.setflags(write=False)
        _cache[key] = (x, ref, tol)
    return _cache[key]


def _check_curve(x, ref, tol, n_fft, hop, label):
    offsets, stds, pad = renoiser.sniff_offset(x, G.SR, n_fft, hop)
    assert stds.dtype == np.float64 and stds.shape == (hop,) and np.array_equal(offsets, np.arange(hop))
    err = np.abs(stds - ref)
    print(label, (n_fft, hop, len(x)), "max err", err.max(), "max err / bound", (err / tol).max(), "curve max", ref.max())
    assert np.all(np.isfinite(stds)) and np.all(stds >= 0)
    assert np.all(err <= tol), (label, int(np.argmax(err / tol)), err.max())
    return stds, pad


@pytest.mark.parametrize("name", list(G.GPU_SHAPES))
@pytest.mark.parametrize("sig", ["noise", "noise_and_tone"])
def test_every_offset_within_the_bound(name, sig):
    n_fft, hop, n = G.GPU_SHAPES[name]
    x, ref, tol = _case(sig, getattr(G, sig), n_fft, hop, n)
    stds, pad = _check_curve(x, ref, tol, n_fft, hop, f"{name}/{sig}")
    # the best pad is the first maximum of the returned curve, and as good as the float64 best up to the arithmetic
    assert pad == int(np.argmax(stds))
    assert ref.max() - ref[pad] <= 2 * tol.max()


@pytest.mark.parametrize("where", ["first", "last", "middle"])
def test_unit_impulse_pins_the_index_map_at_both_reflections(where):
    n_fft, hop, n = G.IMPULSE_SHAPE
    assert any((n + i + n_fft // 2) % hop == 0 for i in range(hop))  # a last frame ends on the reflected x[n - 1]
    at = {"first": 0, "last": n - 1, "middle": n // 2}[where]
    x, ref, tol = _case("impulse_" + where, lambda m: G.impulse(m, at), n_fft, hop, n)
    _check_curve(x, ref, tol, n_fft, hop, "impulse/" + where)


def test_tone_whose_period_divides_the_hop_exercises_the_clamp():
    n_fft, hop, n = G.TONE_SHAPE
    x, ref, tol = _case("tone", G.tone, n_fft, hop, n)
    stds, _ = _check_curve(x, ref, tol, n_fft, hop, "tone")
    assert np.all(np.isfinite(stds)) and np.all(stds >= 0)


def test_interleaved_channel_sentinels_determinism_and_device_input():
    n_fft, hop, n = G.GPU_SHAPES["small"]
    x, ref, tol = _case("noise_and_tone", G.noise_and_tone, n_fft, hop, n)
    _, mono, pad = renoiser.sniff_offset(x, G.SR, n_fft, hop)
    # channel 0 of an interleaved signal whose other channel is NaN: the mono result, bit for bit
    x2 = np.stack((x, np.full(n, np.nan, dtype=np.float32)), axis=1)
    _, st2, pad2 = renoiser.sniff_offset(x2, G.SR, n_fft, hop, channel=0)
    assert np.array_equal(st2, mono) and pad2 == pad
    x2_t = torch.from_numpy(x2).cuda()
    keep = x2_t.clone()
    dev_curve = renoiser.sniff_offset_dev(x2_t, G.SR, n_fft, hop, 0)             # strided read of the interleaved tensor
    assert dev_curve.dtype == torch.float64 and np.array_equal(_dev.to_host(dev_curve), mono)
    assert torch.equal(torch.nan_to_num(x2_t), torch.nan_to_num(keep))           # the input is never modified
    # ... and channel 1 gives NaN (the reference's STFT of NaN is NaN)
    assert np.all(np.isnan(_dev.to_host(renoiser.sniff_offset_dev(x2_t, G.SR, n_fft, hop, 1))))
    # numpy in == device tensor in
    _, st_t, pad_t = renoiser.sniff_offset(torch.from_numpy(x).cuda(), G.SR, n_fft, hop)
    assert isinstance(st_t, np.ndarray) and np.array_equal(st_t, mono) and pad_t == pad
    # stds written into a hop + 2 buffer: the sentinel cells stay
    buf = torch.full((hop + 2,), -7.25, dtype=torch.float64, device="cuda")
    renoiser.sniff_offset_dev(torch.from_numpy(x).cuda(), G.SR, n_fft, hop, 0, out=buf[1:])
    got = _dev.to_host(buf)
    assert got[0] == -7.25 and got[-1] == -7.25 and np.array_equal(got[1:-1], mono)
    # two runs are bit-identical, at a shape with several workgroups too
    n_fft, hop, n = G.GPU_SHAPES["default_chunks_and_tiles"]
    xb, _, _ = _case("noise", G.noise, n_fft, hop, n)
    a = renoiser.sniff_offset(xb, G.SR, n_fft, hop)[1]
    b = renoiser.sniff_offset(xb, G.SR, n_fft, hop)[1]
    assert np.array_equal(a, b)


@pytest.mark.parametrize("fused", [True, False])
def test_renoise_offset_equals_the_padded_call(fused):
    fft, hop, n = 256, 64, 5000
    x = np.stack((G.noise_and_tone(n, seed=5), G.noise(n, seed=6)), axis=1)
    final = np.full(fft // 2 + 1, -26.0)                             # about the noise's own level: some bins gated, some not
    x_t = torch.from_numpy(x).cuda()
    base = renoiser.renoise_dev(x_t, final, 12.0, fft, hop, fused=fused)
    assert torch.equal(renoiser.renoise_dev(x_t, final, 12.0, fft, hop, fused=fused, offset=0), base)
    assert 0 < int(torch.count_nonzero(base != x_t)) and torch.all(torch.isfinite(base))
    for k in (1, hop - 1):
        want = renoiser.renoise_dev(torch.from_numpy(np.pad(x, ((k, 0), (0, 0)))).cuda(), final, 12.0, fft, hop, fused=fused)[k:]
        got = renoiser.renoise_dev(x_t, final, 12.0, fft, hop, fused=fused, offset=k)
        assert got.shape == base.shape and torch.equal(got, want)
        assert not torch.equal(got, base)                            # the frames really moved
        out = torch.empty_like(base)
        assert renoiser.renoise_dev(x_t, final, 12.0, fft, hop, fused=fused, offset=k, out=out) is out and torch.equal(out, want)
    if fused:                                                        # the numpy entry point takes the same path
        k = hop - 1
        want = renoiser.renoise(np.pad(x, ((k, 0), (0, 0))), G.SR, final, 12.0, fft, hop)[k:]
        assert np.array_equal(renoiser.renoise_offset(x, G.SR, final, k, 12.0, fft, hop), want)
        assert np.array_equal(renoiser.renoise_offset(x, G.SR, final, 0, 12.0, fft, hop), renoiser.renoise(x, G.SR, final, 12.0, fft, hop))
