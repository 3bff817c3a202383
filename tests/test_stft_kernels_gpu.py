"""K_stft and K_istft (csrc/stft.hip) at the C ABI against the float64 statements of tests/stft_np.py, compiled variant by compiled
variant: par_stft_f32 (44 kernels), par_stft_big_f32 (eight four-step splits), par_istft_f32 (fused sizes 16 ... 2048, the frame
array path, eight big sizes).  The case tables, the metrics and the bounds live in stft_np and are checked by
tests/test_stft_inputs_cpu.py, which also shows that the metrics reject a 1e-5 twiddle error in one bin, a swapped bin pair, a frame
one sample late, an ignored stride, a quiet passage carrying a loud one 60 dB down and an honoured Im X[0].

STFT: per frame, max_k |got - want| / max_k |want| <= R x yardstick(M); a frame of zeros comes out as exact zeros (1e-7f in mode 1).
ISTFT: per block of hop x Frames samples (a workgroup's stride), in overlap-add units, <= R x iyardstick(n_fft); gaps between frames
(hop > n_fft) and everything beyond the overlap-add length are +0.0 bit for bit.  Every call runs twice on fresh guarded buffers:
the two results are bit-identical, the guards and the pitch padding still hold the sentinel, and no input changed.

Each test prints kernel error / yardstick (pytest -s); the worst per size and entry point are in NOTES.md, "STFT / ISTFT at the ABI",
and R in stft_np is 3 x the worst, rounded up to the next integer."""
import numpy as np
import pytest

import stft_np as N

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
    p.ratios = {}
    yield p
    for (entry, M), r in sorted(p.ratios.items()):
        print(f"\nRATIO {entry:6s} M={M:8d} worst error / yardstick = {r:.3f}", end="")
    print()


def note(par, entry, M, ratio):
    par.ratios[(entry, M)] = max(par.ratios.get((entry, M), 0.0), float(ratio))


def unique(cases, key):
    seen = {}
    for c in cases:
        seen.setdefault(key(c), []).append(c)
    return list(seen.items())


# ------------------------------------------------------------------------------------------------ forward
def run_stft(par, c, x, big=False, x_guard=64):
    """one guarded call -> (spectrum (frames, bins) complex64 or float32, every float32 cell of the output buffer)"""
    M = c.n_fft * c.zp
    bins, cells = M // 2 + 1, 2 if c.mode == 0 else 1
    nf = N.n_frames_of(c.n, c.n_fft, c.hop)
    assert nf == par.L.par_stft_frames(c.n, c.n_fft, c.hop)
    pitch_arg = N.pitch_of(c.pitch, bins)
    pitch = pitch_arg or bins
    xs = N.Guarded(par.torch, c.n * c.stride, N.interleave(x, c.stride), guard=x_guard)
    win = N.Guarded(par.torch, c.n_fft, N.window32(c.win, c.n_fft))
    out = N.Guarded(par.torch, nf * pitch * cells)
    if big:
        need = int(par.L.par_stft_big_scratch_bytes(c.n, c.n_fft, c.hop, c.zp))
        assert need > 0 and need % 4 == 0 and pitch_arg == 0
        scratch = N.Guarded(par.torch, need // 4)
        args = (par.dev, xs.ptr(), c.n, c.stride, c.n_fft, c.hop, c.zp, win.ptr(), out.ptr(), c.mode, scratch.ptr())
        assert par.L.par_stft_big_f32(*args, need - 1, par.stream()) == 4                  # a scratch one byte short is refused
        par.check(par.L.par_stft_big_f32(*args, need, par.stream()))
    else:
        par.check(par.L.par_stft_f32(par.dev, xs.ptr(), c.n, c.stride, c.n_fft, c.hop, c.zp, win.ptr(), out.ptr(), c.mode, pitch_arg, par.stream()))
    par.torch.cuda.synchronize()
    flat, ok = out.read()
    assert ok, ("output guards", c)
    assert xs.unchanged() and win.unchanged(), ("inputs changed", c)
    if big:
        assert scratch.read()[1], ("scratch guards", c)
    rows = flat.reshape(nf, pitch * cells)
    assert N.is_sentinel(rows[:, bins * cells:]).all(), ("pitch padding written", c)
    assert not N.is_sentinel(rows[:, :bins * cells]).any(), ("cells not written", c)
    body = np.ascontiguousarray(rows[:, :bins * cells])
    return (body.view(np.complex64) if c.mode == 0 else body), flat


def check_stft(par, c, entry, R, big=False):
    x, S = N.scase_reference(c.n_fft, c.zp, c.hop, c.n, c.win, c.sig, c.seed)
    M = c.n_fft * c.zp
    got, flat = run_stft(par, c, x, big)
    _, flat2 = run_stft(par, c, x, big)
    assert np.array_equal(flat.view(np.uint32), flat2.view(np.uint32)), ("two runs differ", c)
    if c.mode == 0:
        e = N.frame_err(got, S)
    else:
        e = N.frame_err(got, N.mag64(S), 1e-7, N.MAG_ULP)
    worst = float(np.max(e))
    print(f"\n{entry} {c.group} n_fft={c.n_fft} zp={c.zp} hop={c.hop} n={c.n} mode={c.mode} stride={c.stride} {c.pitch} {c.win} {c.sig}: "
          f"{len(e)} frames, worst {worst:.3g} = {worst / N.yardstick(M):.2f} yardsticks (frame {int(np.argmax(e))})", end="")
    assert worst <= N.bound(R, M), (c, worst, N.bound(R, M), int(np.argmax(e)))
    note(par, entry, M, worst / N.yardstick(M))
    return got, flat


REG = unique(N.stft_reg_cases(), lambda c: (c.group, c.n_fft, c.zp, c.hop, c.n, c.win, c.sig))


@pytest.mark.parametrize("key,cases", REG, ids=["-".join(str(v) for v in k) for k, _ in REG])
def test_par_stft_f32(par, key, cases):
    for c in cases:
        check_stft(par, c, "reg", N.R_REG)


BIG = unique(N.stft_big_cases(), lambda c: (c.group, c.n_fft, c.zp, c.mode))


@pytest.mark.parametrize("key,cases", BIG, ids=["-".join(str(v) for v in k) for k, _ in BIG])
def test_par_stft_big_f32(par, key, cases):
    for c in cases:
        got, flat = check_stft(par, c, "four", N.R_FOUR, big=True)
        if c.stride == 1:                                      # the signal 4 bytes off the 8-byte grid: the same bits
            x, _ = N.scase_reference(c.n_fft, c.zp, c.hop, c.n, c.win, c.sig, c.seed)
            _, off = run_stft(par, c, x, big=True, x_guard=65)
            assert np.array_equal(off.view(np.uint32), flat.view(np.uint32)), ("misaligned signal", c)


# ------------------------------------------------------------------------------------------------ inverse
def run_istft(par, c, S):
    skip, y_len, ola = N.icase_geometry(c)
    bins = c.n_fft // 2 + 1
    spec = N.Guarded(par.torch, S.size * 2, S, guard=4 * bins)             # rows beyond n_frames hold the NaN sentinel
    win = N.Guarded(par.torch, c.n_fft, N.window32(c.win, c.n_fft))
    y = N.Guarded(par.torch, y_len)
    need = int(par.L.par_istft_scratch_floats(c.n_frames, c.n_fft, c.hop))
    assert (need == 0) == (N.istft_variant(c.n_fft, c.hop)[0] == "fused"), c
    frames = N.Guarded(par.torch, need) if need else None
    par.check(par.L.par_istft_f32(par.dev, spec.ptr(), c.n_frames, c.n_fft, c.hop, win.ptr(), frames.ptr() if need else None, y.ptr(),
                                  y_len, skip, par.stream()))
    par.torch.cuda.synchronize()
    got, ok = y.read()
    assert ok, ("output guards", c)
    assert spec.unchanged() and win.unchanged(), ("inputs changed", c)
    assert need == 0 or frames.read()[1], ("scratch guards", c)
    return got


ICASES = N.istft_cases()


@pytest.mark.parametrize("c", ICASES, ids=["-".join(str(v) for v in c[:7]) + "-" + c.sig for c in ICASES])
def test_par_istft_f32(par, c):
    S, ref = N.icase_reference(c)
    skip, y_len, ola = N.icase_geometry(c)
    got = run_istft(par, c, S)
    assert np.array_equal(got.view(np.uint32), run_istft(par, c, S).view(np.uint32)), ("two runs differ", c)
    assert not N.is_sentinel(got).any(), ("samples not written", c)
    big = c.n_fft > 8192
    b, yard = N.bound(N.R_IBIG if big else N.R_ISTFT, c.n_fft, inverse=True), N.iyardstick(c.n_fft)
    TT = np.arange(y_len, dtype=np.int64) + skip
    beyond = TT >= ola
    assert np.all(got.view(np.uint32)[beyond] == 0), ("beyond the overlap-add length", c, np.flatnonzero(beyond & (got.view(np.uint32) != 0))[:5])
    gap = ~beyond & (TT % c.hop >= c.n_fft)                    # hop > n_fft: no frame covers the sample
    assert np.all(got.view(np.uint32)[gap] == 0), ("gap samples", c, np.flatnonzero(gap & (got.view(np.uint32) != 0))[:5], got[gap][:5])
    assert np.all(ref.y[:y_len][gap] == 0) and np.all(ref.y[:y_len][beyond] == 0)
    want_u = N.ola_units(ref.y, ref.env)
    got_u = want_u.copy()                                      # samples the call did not ask for: the reference's own (no error, but
    got_u[:y_len] = N.ola_units(got, ref.env[:y_len])          # their peak counts: a one-sample output has none of its own)
    block = c.hop * N.istft_frames_per_group(c.n_fft)
    e = N.block_err(got_u, want_u, block, reach=c.n_fft - 1)
    print(f"\n{'ibig' if big else 'istft'} {c.group} n_fft={c.n_fft} hop={c.hop} frames={c.n_frames} {c.win} skip={skip} y_len={y_len} {c.sig}: "
          f"{e:.3g} = {e / yard:.2f} yardsticks", end="")
    assert e <= b, (c, e, b)
    note(par, "ibig" if big else "istft", c.n_fft, e / yard)
    if c.group == "count":                                     # the samples where one envelope path hands over to the next, one by one
        assert skip == 0
        for t in sorted({c.n_fft - 2, c.n_fft - 1, c.n_fft, c.hop * (c.n_frames - 1) - 1, c.hop * (c.n_frames - 1), c.hop * (c.n_frames - 1) + 1}):
            if 0 <= t < y_len:
                peak = float(np.max(np.abs(want_u[max(t - c.n_fft + 1, 0):t + c.n_fft])))
                assert abs(got_u[t] - want_u[t]) <= b * peak, (c, t, got[t], ref.y[t], ref.env[t])
    if c.group == "zero_env":                                  # env = 0 exactly: not divided, and 0 x frame is 0
        assert np.all(got[::c.hop][:c.n_frames] == 0.0)
