"""K_gauge at the C ABI (par_gauge_frames, par_gauge_scratch_bytes, par_gauge_offset_f32 of csrc/gauge.hip) against the exact
oracles of tests/gauge_inputs.py, where test_gauge_gpu.py -- the Python wrapper, one filter, a bound on float32 rounding -- does
not reach: index arithmetic.  Integer signals and filters make every tap sum and both moments exact, so the variance is compared
with a Fraction under a tolerance of 8 float64 roundings (gauge_inputs' docstring derives it); delta filters read single samples of
the padded signal; a real filter is compared with the exact float32 FMA chain.  tests/test_gauge_inputs_cpu.py proves the inputs'
preconditions and that this tolerance sees a lost, doubled or misfiled frame on every pad it touches.

Every call: stds lies between sentinel cells; scratch is exactly par_gauge_scratch_bytes long, filled with NaN bit patterns (as
float64 and as float32) and followed by guard cells; x, h_re and h_im lie between NaN guard rows and must be unchanged afterwards;
every case runs twice and must repeat bit for bit.  pytest -s prints the measured worst error / bound (NOTES.md)."""
from fractions import Fraction

import numpy as np
import pytest

import gauge_inputs as I
import gauge_np as G
from test_heal_kernels_gpu import Guarded, bits

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5
SCRATCH_GUARD = -7.25
IDS = [I.shape_id(s) for s in I.ALL_SHAPES]


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


def gauge(par, shape, x, h_re, h_im, stride=1, channel=0):
    """stds of channel `channel` of x (n,) or (n, stride), from two guarded runs that must agree bit for bit"""
    n_fft, hop, n = shape
    body = np.asarray(x, dtype=np.float32).reshape(n, stride)
    need = int(par.L.par_gauge_scratch_bytes(n, n_fft, hop))
    assert need > 0 and need % 8 == 0
    for off in (0, hop - 1):
        assert par.L.par_gauge_frames(n, n_fft, hop, off) == I.frames(n, n_fft, hop, off)
    gx = Guarded(par, body, 2, np.float32(np.nan))
    gr = Guarded(par, np.asarray(h_re, dtype=np.float32), 4, np.float32(np.nan))
    gi = Guarded(par, np.asarray(h_im, dtype=np.float32), 4, np.float32(np.nan))
    poison = np.full(need // 8, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64).view(np.float64)     # NaN as float64 and as two float32
    got = []
    for _ in range(2):
        out = Guarded(par, np.full(hop, SENTINEL), 2, SENTINEL)
        scratch = Guarded(par, poison, 4, SCRATCH_GUARD)
        par.check(par.L.par_gauge_offset_f32(par.dev, gx.ptr(channel), n, stride, n_fft, hop, gr.ptr(), gi.ptr(), out.ptr(),
                                             scratch.ptr(), need, par.stream()))
        par.torch.cuda.synchronize()
        got.append(out.read().copy())
        assert out.guards_intact() and scratch.guards_intact()
    assert np.array_equal(bits(got[0]), bits(got[1]))
    assert gx.unchanged() and gr.unchanged() and gi.unchanged()
    return got[0]


def worst_over_bound(got, per_pad, label):
    """largest |got^2 - var| / tolerance over the pads, asserted <= 1"""
    assert got.shape == (len(per_pad),) and np.all(np.isfinite(got)) and np.all(got >= 0), label
    ratios = [I.error_over_bound(g, m) for g, m in zip(got, per_pad)]
    k = int(np.argmax(ratios))
    assert ratios[k] <= 1.0, (label, "pad", k, "got", float(got[k]), "want", float(I.variance(per_pad[k])) ** 0.5, ratios[k])
    return ratios[k]


@pytest.mark.parametrize("shape", I.ALL_SHAPES, ids=IDS)
def test_integer_filter_exact_variance(par, shape):
    c = I.int_case(shape)
    got = gauge(par, shape, c.x, c.h_re, c.h_im)
    worst = worst_over_bound(got, c.moments, shape)
    print(f"\nK_gauge integers {shape}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("shape", I.shapes_of(*I.DELTA_GROUPS) + [G.IMPULSE_SHAPE],
                         ids=[I.shape_id(s) for s in I.shapes_of(*I.DELTA_GROUPS) + [G.IMPULSE_SHAPE]])
def test_delta_filter_reads_the_padded_signal(par, shape):
    x, per_filter = I.delta_moments(shape)
    worst = 0.0
    for (m, part), per_pad in per_filter.items():
        got = gauge(par, shape, x, *I.delta_filter(shape[0], m, part))
        worst = max(worst, worst_over_bound(got, per_pad, (shape, "tap", m, "part", part)))
    print(f"\nK_gauge deltas {shape}: {len(per_filter)} filters, worst error / bound {worst:.3f}")


@pytest.mark.parametrize("shape", I.shapes_of("hop_over_tile", "final_runs"),
                         ids=[I.shape_id(s) for s in I.shapes_of("hop_over_tile", "final_runs")])
def test_zero_signal_gives_exact_zeros(par, shape):
    """with the scratch full of NaN: no partial and no edge cell is read that this call did not write"""
    c = I.int_case(shape)
    got = gauge(par, shape, np.zeros(shape[2], dtype=np.float32), c.h_re, c.h_im)
    assert np.array_equal(bits(got), np.zeros(shape[1], dtype=np.uint64))


@pytest.mark.parametrize("shape", I.shapes_of("rotation", "no_dense"), ids=[I.shape_id(s) for s in I.shapes_of("rotation", "no_dense")])
@pytest.mark.parametrize("stride", [2, 3])
def test_strided_channel_equals_the_packed_signal(par, shape, stride):
    c = I.int_case(shape)
    packed = gauge(par, shape, c.x, c.h_re, c.h_im)
    worst_over_bound(packed, c.moments, shape)
    for channel in (0, stride - 1):
        body = np.full((shape[2], stride), np.nan, dtype=np.float32)
        body[:, channel] = c.x
        got = gauge(par, shape, body, c.h_re, c.h_im, stride=stride, channel=channel)
        assert np.array_equal(bits(got), bits(packed)), (shape, stride, channel)


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_one_non_finite_sample_makes_every_pad_nan(par, value):
    """NaN as numpy's std gives it; +inf too: inf - mean(inf) is NaN there, and here sum |z|^2 / F - |mean|^2 is inf - inf"""
    (shape,) = I.SHAPES["rotation"]
    c = I.int_case(shape)
    assert shape[1] <= shape[0]                                      # the frames of every pad cover every sample
    for at in (0, shape[2] // 2, shape[2] - 1):
        x = c.x.copy()
        x[at] = value
        got = gauge(par, shape, x, c.h_re, c.h_im)
        assert np.all(np.isnan(got)), (value, at, got)
        if at == shape[2] // 2:
            with np.errstate(all="ignore"):
                z = G.frames_of(G.padded(x, 3, shape[0]), shape[0], shape[1]) @ (c.h_re.astype(np.float64) + 1j * c.h_im)
                assert np.isnan(np.std(z))


@pytest.mark.parametrize("name", I.REAL_SHAPES)
def test_real_filter_equals_the_exact_fma_chain(par, name):
    """renoiser.gauge_filter rounded to float32 on noise_and_tone: z is ONE float32 FMA chain over ascending m per part, which the
    emulation reproduces bit for bit, so only the float64 moments differ: 18 * 2^-53 * mean |z|^2 on the variance, the figure of
    gauge_np.bound's derivation (two compensated sums, a tree of depth 8, six operations)."""
    shape = G.GPU_SHAPES[name]
    x, hr, hi, z, repaired, _ = I.real_case(name)
    got = gauge(par, shape, x, hr, hi)
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    worst = 0.0
    for i, (zr, zi) in enumerate(z):
        sr, si, s2, F = I.float_moments(zr, zi)
        assert F == I.frames(shape[2], shape[0], shape[1], i)
        var, tol = s2 / F - (sr * sr + si * si) / (F * F), 18 * I.U64 * s2 / F
        ratio = float(abs(Fraction(float(got[i])) ** 2 - var) / tol)
        assert ratio <= 1.0, (name, i, float(got[i]), float(var) ** 0.5, ratio)
        worst = max(worst, ratio)
    print(f"\nK_gauge real filter {name} {shape}: worst error / bound {worst:.4f} ({repaired} emulation steps repaired)")
