"""par_sosfiltfilt_f64 and par_sosfiltfilt_batch_f64 at the C ABI, on the GPU, against the long-double oracle.

Every (cascade, signal, length) of filt_inputs.py goes through the single form and through two batches of three rows (one cascade
for all rows; three different narrow cascades, one per row), the rows at strides above n between sentinel cells.  With
    e_gpu   = max |y - oracle| / max |oracle|        e_scipy = the same for scipy.signal.sosfiltfilt on the same input
the assertion is  e_gpu <= R * max(e_scipy, 8 * 2^-53):  the kernels may lose R times what scipy's own float64 recurrence loses on
that input, whatever the conditioning of the band.  R = filt_inputs.R = 15 = 3 x the worst ratio measured on the MI355X, 4.97
(NOTES.md, "K_sosfiltfilt against a long-double oracle", holds the ratios per cascade: of this build, of the build with exact
block matrices but plain chain sums -- up to 83 -- and of the build before either -- up to 10^5).  The CPU restatement of the
same algorithm (test_filt_cpu.py) stays below 2."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.signal

import filt_inputs as FI
from oracle import oracle_c

pytestmark = pytest.mark.gpu

R = FI.R
SENT = -7.25                     # sentinel between and around the rows
GUARD = 64


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


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _dp(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + 8 * offset)


@functools.lru_cache(maxsize=None)
def _zi(name):
    return np.ascontiguousarray(scipy.signal.sosfilt_zi(_cascade(name).sos), dtype=np.float64)


def _cascade(name):
    return next(c for c in FI.cascades() + FI.narrow_trio() if c.name == name)


@functools.lru_cache(maxsize=16)
def reference(cname, sname, n):
    """(x, oracle, e_scipy), computed once per case and handed out read-only (the last few cases are kept, not all: 10^8 doubles)"""
    c = _cascade(cname)
    x = FI.signal(sname, n, c.padlen)
    ref = oracle_c.sosfiltfilt_ld(c.sos, x, c.padlen)
    e_scipy = FI.rel_err(scipy.signal.sosfiltfilt(c.sos, x), ref)
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref, e_scipy


def run_single(par, c, x_t):
    """par_sosfiltfilt_f64 on a device signal -> device result; the result and the workspace lie between guard cells"""
    t = par.torch
    n = x_t.numel()
    wl = int(par.L.par_sosfiltfilt_work_len(n, c.padlen))
    work = t.full((wl + GUARD,), SENT, dtype=t.float64, device="cuda:0")
    y = t.full((n + 2 * GUARD,), SENT, dtype=t.float64, device="cuda:0")
    par.check(par.L.par_sosfiltfilt_f64(0, _hp(c.sos), _hp(_zi(c.name)), c.sos.shape[0], _dp(x_t), n, c.padlen, _dp(work), wl,
                                        _dp(y, GUARD), par.stream()))
    assert bool((y[:GUARD] == SENT).all()) and bool((y[GUARD + n:] == SENT).all()), "single form wrote outside y"
    assert bool((work[wl:] == SENT).all()), "single form wrote behind its workspace"
    return y[GUARD:GUARD + n]


def run_batch(par, cs, rows_t, pad_x=5, pad_y=7):
    """par_sosfiltfilt_batch_f64 on len(rows_t) device signals of one length; cs: one cascade for all rows or one per row.
    x rows are x_stride = n + pad_x apart with NaN between them (a read of the gap would show), y rows y_stride = n + pad_y apart
    with sentinels between them that must survive.  -> device results [rows][n]"""
    t = par.torch
    n_sig, n = len(rows_t), rows_t[0].numel()
    padlen, n_sec = cs[0].padlen, cs[0].sos.shape[0]
    xs, ys = n + pad_x, n + pad_y
    x = t.full((n_sig, xs), float("nan"), dtype=t.float64, device="cuda:0")
    for i, r in enumerate(rows_t):
        x[i, :n] = r
    y = t.full((GUARD + n_sig * ys + GUARD,), SENT, dtype=t.float64, device="cuda:0")
    sos = np.ascontiguousarray([c.sos for c in cs], dtype=np.float64)
    zi = np.ascontiguousarray([_zi(c.name) for c in cs], dtype=np.float64)
    wl = int(par.L.par_sosfiltfilt_batch_work_len(n, padlen, n_sig, n_sec))
    work = t.full((wl + GUARD,), SENT, dtype=t.float64, device="cuda:0")
    par.check(par.L.par_sosfiltfilt_batch_f64(0, _hp(sos), _hp(zi), len(cs), n_sec, _dp(x), xs, n_sig, n, padlen, _dp(work), wl,
                                              _dp(y, GUARD), ys, par.stream()))
    body = y[GUARD:GUARD + n_sig * ys].view(n_sig, ys)
    assert bool((y[:GUARD] == SENT).all()) and bool((y[GUARD + n_sig * ys:] == SENT).all()), "batched form wrote outside y"
    assert bool((body[:, n:] == SENT).all()), "batched form wrote between the rows of y"
    assert bool((work[wl:] == SENT).all()), "batched form wrote behind its workspace"
    return body[:, :n]


def measure_cascade(par, cname, labels=None, on_case=None):
    """every signal at every length through the single form and a one-cascade batch of three rows (the signal and the two
    after it in SIGNAL_NAMES).  -> [(label, signal, e_gpu, e_scipy, rows_equal, repeat_equal)]"""
    t = par.torch
    c = _cascade(cname)
    out = []
    for label, n in FI.lengths(c.padlen):
        if labels is not None and label not in labels:
            continue
        refs = [reference(cname, s, n) for s in FI.SIGNAL_NAMES]
        x_t = [t.from_numpy(r[0].copy()).to("cuda:0") for r in refs]
        singles = [run_single(par, c, x) for x in x_t]
        again = run_single(par, c, x_t[0])
        for i, sname in enumerate(FI.SIGNAL_NAMES):
            pick = [i, (i + 1) % 4, (i + 2) % 4]
            rows = run_batch(par, [c], [x_t[j] for j in pick])
            rows_equal = all(t.equal(rows[k], singles[j]) for k, j in enumerate(pick))
            repeat_equal = t.equal(again, singles[0]) and t.equal(run_batch(par, [c], [x_t[j] for j in pick]), rows)
            e_gpu = FI.rel_err(singles[i].cpu().numpy(), refs[i][1])
            out.append((label, sname, e_gpu, refs[i][2], rows_equal, repeat_equal))
            if on_case:
                on_case(out[-1])
    return out


def measure_trio(par, labels=None):
    """the three narrow order-3 band-passes as ONE batch, row k filtered by cascade k, every signal at every length.
    -> [(label, signal, cascade, e_gpu, e_scipy, row_equal)]"""
    t = par.torch
    trio = FI.narrow_trio()
    out = []
    for label, n in FI.lengths(21):
        if labels is not None and label not in labels:
            continue
        for sname in FI.SIGNAL_NAMES:
            refs = [reference(c.name, sname, n) for c in trio]
            x_t = t.from_numpy(refs[0][0].copy()).to("cuda:0")
            rows = run_batch(par, list(trio), [x_t, x_t, x_t], pad_x=3, pad_y=1)
            for k, c in enumerate(trio):
                same = t.equal(rows[k], run_single(par, c, x_t))
                out.append((label, sname, c.name, FI.rel_err(rows[k].cpu().numpy(), refs[k][1]), refs[k][2], same))
    return out


def ratio(e_gpu, e_scipy):
    return e_gpu / max(e_scipy, FI.FLOOR)


@pytest.mark.parametrize("cname", FI.CASCADE_NAMES)
def test_both_forms_against_the_oracle(par, cname):
    res = measure_cascade(par, cname)
    assert len(res) == len(FI.SIGNAL_NAMES) * len(FI.LENGTH_LABELS)
    worst = max(res, key=lambda r: ratio(r[2], r[3]))
    print(f"{cname}: worst e_gpu / max(e_scipy, floor) = {ratio(worst[2], worst[3]):.2f} at {worst[0]} {worst[1]} "
          f"(e_gpu {worst[2]:.2e}, e_scipy {worst[3]:.2e})")
    for label, sname, e_gpu, e_scipy, rows_equal, repeat_equal in res:
        assert e_gpu <= R * max(e_scipy, FI.FLOOR), (cname, label, sname, e_gpu, e_scipy, ratio(e_gpu, e_scipy))
        assert rows_equal, (cname, label, sname, "a batch row differs from the single call")
        assert repeat_equal, (cname, label, sname, "two runs differ")


def test_batch_of_three_narrow_cascades(par):
    res = measure_trio(par)
    assert len(res) == 3 * len(FI.SIGNAL_NAMES) * len(FI.LENGTH_LABELS)
    worst = max(res, key=lambda r: ratio(r[3], r[4]))
    print(f"trio: worst ratio {ratio(worst[3], worst[4]):.2f} at {worst[:3]} (e_gpu {worst[3]:.2e}, e_scipy {worst[4]:.2e})")
    for label, sname, cname, e_gpu, e_scipy, same in res:
        assert e_gpu <= R * max(e_scipy, FI.FLOOR), (cname, label, sname, e_gpu, e_scipy, ratio(e_gpu, e_scipy))
        assert same, (cname, label, sname, "a batch row differs from the single call")


@pytest.mark.parametrize("cname", ("band_300_3000_48k_o3", "low_2_44k_o3", "one_section_low"))
def test_index_map_at_the_ends_and_the_seams(par, cname):
    """One unit sample at the places where an index of the odd extension, of the reversed pass or of the trim could slip by one:
    x[0] and x[n-1] (doubled by the extension), x[padlen] and x[n-1-padlen] (the last samples the extension mirrors), x[1], and
    the first sample of a block.  A slip moves the response by a sample -- orders of magnitude beyond R e_scipy against the
    oracle; the seam impulse's response also peaks where the oracle's does, which on the wide cascades is the impulse itself."""
    t = par.torch
    c = _cascade(cname)
    for label, n in (("L769", 3 * FI.BLOCK + 1 - 2 * c.padlen), ("L65537", dict(FI.lengths(c.padlen))["L65537"])):
        seam = FI.seam_index(n, c.padlen)
        assert (seam + c.padlen) % FI.BLOCK == 0
        for at in (0, 1, c.padlen, seam, n - 1 - c.padlen, n - 1):
            x = np.zeros(n)
            x[at] = 1.0
            ref = oracle_c.sosfiltfilt_ld(c.sos, x, c.padlen)
            e_scipy = FI.rel_err(scipy.signal.sosfiltfilt(c.sos, x), ref)
            y = run_single(par, c, t.from_numpy(x).to("cuda:0")).cpu().numpy()
            e_gpu = FI.rel_err(y, ref)
            print(f"{cname} {label} impulse at {at}: e_gpu {e_gpu:.2e} e_scipy {e_scipy:.2e}")
            assert e_gpu <= R * max(e_scipy, FI.FLOOR), (cname, label, at, e_gpu, e_scipy)
            if at == seam:
                assert int(np.argmax(np.abs(y))) == int(np.argmax(np.abs(ref)))
                if not c.narrow and label == "L65537":
                    assert int(np.argmax(np.abs(y))) == seam


@pytest.mark.parametrize("cname", ("low_2_44k_o3", "golden_low_20_172", "one_section_low"))
def test_low_pass_returns_a_ramp(par, cname):
    """The odd extension continues a ramp, and a low-pass has unit gain and (forward-backward) no delay at DC: away from the
    settling of sosfilt_zi's step state the ramp comes back.  How far the EXACT result is from the ramp is the oracle's figure
    d_oracle; the kernel's result must be no further than that plus R e_scipy."""
    t = par.torch
    c = _cascade(cname)
    for label, n in FI.lengths(c.padlen):
        x, ref, e_scipy = reference(cname, "ramp", n)
        y = run_single(par, c, t.from_numpy(x.copy()).to("cuda:0")).cpu().numpy()
        peak = float(np.max(np.abs(ref)))
        d_gpu, d_oracle = float(np.max(np.abs(y - x))) / peak, float(np.max(np.abs(ref - x))) / peak
        print(f"{cname} {label}: |y - ramp| {d_gpu:.2e}, |oracle - ramp| {d_oracle:.2e}, e_scipy {e_scipy:.2e}")
        assert d_gpu <= d_oracle + R * max(e_scipy, FI.FLOOR), (cname, label, d_gpu, d_oracle, e_scipy)


def test_narrow_band_through_the_tiled_kernels(par):
    """L >= 2 10^7: the single form runs the LDS-tiled block kernels and the two-level chain over 306 super-blocks, here on the
    20-40 Hz band.  The ratio assertion on every 997th output and the first and last 4096."""
    t = par.torch
    c = _cascade("band_20_40_48k_o3")
    n = 20_000_003
    assert n + 2 * c.padlen >= 20_000_000
    x = np.random.default_rng(77).standard_normal(n) + 0.5
    idx = np.unique(np.concatenate([np.arange(4096), np.arange(0, n, 997), np.arange(n - 4096, n)]))
    ref = oracle_c.sosfiltfilt_ld(c.sos, x, c.padlen)[idx]
    e_scipy = FI.rel_err(scipy.signal.sosfiltfilt(c.sos, x)[idx], ref)
    y = run_single(par, c, t.from_numpy(x).to("cuda:0"))[t.from_numpy(idx).to("cuda:0")].cpu().numpy()
    e_gpu = FI.rel_err(y, ref)
    print(f"tiled, 20-40 Hz, n = {n}: e_gpu {e_gpu:.2e}, e_scipy {e_scipy:.2e}, ratio {ratio(e_gpu, e_scipy):.2f}")
    assert e_gpu <= R * max(e_scipy, FI.FLOOR), (e_gpu, e_scipy, ratio(e_gpu, e_scipy))
