"""The six entry points of csrc/heal.hip at the C ABI, cell by cell, against the float64 oracles of tests/heal_inputs.py -- where the
end-to-end heal tests of test_hip_parity.py (STFT -> kernels -> ISTFT, an error relative to the file's peak) do not reach: band widths
around the 256-thread geometry of k_inpaint_gain / k_apply_gain_boxes, surrounding frames and box lengths against the P frame lanes,
boxes flush with the spectrogram's ends, bin 0 and the last bin, skipped markers, a pre-set and a reused mask, poison values,
k_copy_segments on short segments and reflections over several periods, k_curve_scale on knots.

Every buffer a kernel reads or writes lies INSIDE a larger tensor with guard rows on both sides and the kernel gets an interior
pointer: an index error lands in a guard and fails an assertion.  Each test ends by checking its guards bit for bit.
tests/test_heal_inputs_cpu.py proves that no cell of the inputs sits within 1e-6 dB of a clip, so `written or not` and `clipped or not`
cannot differ legitimately.  pytest -s prints the measured figures (NOTES.md, K_heal)."""
import ctypes

import numpy as np
import pytest

import heal_inputs as H

pytestmark = pytest.mark.gpu

TOL = 1e-5                  # the BASELINE contract, here per bin: relative to that bin's own magnitude
BAND_TOL = 1e-10            # dB; the project's bound for this quantity (test_expander_gpu.py::test_fused_band_db_equals_composed)
BIT_EQUAL_SHARE = 0.999


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


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.real.dtype.itemsize])


class Guarded:
    """`body` (rows, ...) between `guard` rows of `fill` on either side, on the device; ptr() points at the body's first row"""

    def __init__(self, par, body, guard, fill):
        body = np.ascontiguousarray(body)
        self.g, self.rows = int(guard), body.shape[0]
        whole = np.full((self.rows + 2 * self.g,) + body.shape[1:], fill, dtype=body.dtype)
        whole[self.g:self.g + self.rows] = body
        self.before = whole
        self.t = par.torch.from_numpy(whole.copy()).cuda()

    def ptr(self, offset=0):
        return ctypes.c_void_p(self.t[self.g].data_ptr() + offset * self.t.element_size())

    def read(self):
        self.now = self.t.cpu().numpy()
        return self.now[self.g:self.g + self.rows]

    def guards_intact(self):
        now = self.t.cpu().numpy()
        g, r = self.g, self.rows
        return np.array_equal(bits(now[:g]), bits(self.before[:g])) and np.array_equal(bits(now[g + r:]), bits(self.before[g + r:]))

    def unchanged(self):
        return np.array_equal(bits(self.t.cpu().numpy()), bits(self.before))


def dev_i(par, a, dtype):
    return par.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


SPEC_SENTINEL = np.complex64(1e3 + 1e3j)


class Heal:
    """spectrogram and mask of a case between guards, the two entry points on them"""

    def __init__(self, par, c, spec=None, preset=None):
        self.par, self.c = par, c
        g = H.max_fs(c) + 2
        self.spec = Guarded(par, c.spec if spec is None else spec, g, SPEC_SENTINEL)
        self.mask = Guarded(par, np.zeros(c.spec.shape, np.float32) if preset is None else preset, g, np.float32(0))

    def _call(self, fn, markers):
        m = dev_i(self.par, np.asarray(markers, dtype=np.int32).reshape(-1, 5), np.int32)
        p = self.par
        p.check(fn(p.dev, self.spec.ptr(), self.c.frames, self.c.bins, ctypes.c_void_p(m.data_ptr()), len(markers), self.mask.ptr(),
                   p.stream()))
        p.torch.cuda.synchronize()

    def inpaint(self, markers=None):
        self._call(self.par.L.par_inpaint_gain_db_c64, self.c.markers if markers is None else markers)
        return self.mask.read().copy()

    def apply(self, markers=None):
        self._call(self.par.L.par_spec_apply_gain_boxes_c64, self.c.markers if markers is None else markers)
        return self.spec.read().copy()

    def new_spec(self):
        self.spec = Guarded(self.par, self.c.spec, self.spec.g, SPEC_SENTINEL)


def check_mask(c, dev, ref, preset=None):
    """-> (worst |dev - float64 ref| dB, cells inside boxes, of them bit-equal to float32(ref))"""
    assert dev.dtype == np.float32 and dev.shape == ref.shape
    ref32 = ref.astype(np.float32)
    err = np.abs(dev.astype(np.float64) - ref32.astype(np.float64))
    tol = np.maximum(np.spacing(np.abs(ref32)).astype(np.float64), 1e-9)
    bad = np.argwhere(~(err <= tol))
    assert len(bad) == 0, (c, len(bad), bad[:5].tolist(), dev[tuple(bad[0])], ref[tuple(bad[0])])
    inside = H.box_cells(ref.shape, c.markers)
    outside = np.zeros(ref.shape, np.float32) if preset is None else np.asarray(preset)
    assert np.array_equal(bits(dev[~inside]), bits(outside[~inside])), c       # outside every box, and every skipped marker: untouched
    assert np.array_equal(dev > 0, ref > 0), c
    equal = int(np.sum(bits(dev[inside]) == bits(ref32[inside])))
    n = int(inside.sum())
    assert equal >= BIT_EQUAL_SHARE * n, (c, equal, n)
    return float(np.max(np.abs(dev.astype(np.float64) - ref), initial=0.0)), n, equal


# ------------------------------------------------------------------------------------------ inpaint
@pytest.mark.parametrize("name", H.NAMED)
def test_inpaint_mask_named(par, name):
    c = H.case(name)
    h = Heal(par, c, preset=c.preset)
    dev = h.inpaint()
    ref = H.gain_mask_np(c.spec, c.markers, c.preset)
    worst, n, equal = check_mask(c, dev, ref, c.preset)
    print(f"\n{name}: geometry {H.kernel_geometry([m for m in c.markers if H.marker_valid(m, c.frames, c.bins)][0])}; worst "
          f"|mask - float64| {worst:.2e} dB, {equal} of {n} box cells bit-equal to float32(ref)")
    if c.preset is not None:
        new = H.gain_mask_np(c.spec, c.markers).astype(np.float32)
        assert np.array_equal(dev, np.maximum(np.asarray(c.preset), new))
    if c.expect.get("none_written"):
        assert not dev.any()
    if c.expect.get("all_clipped"):
        assert np.all(dev[H.box_cells(dev.shape, c.markers)] == np.float32(255))
    # the order of the markers does not matter: bit for bit
    if len(c.markers) > 1:
        order = np.random.default_rng(5).permutation(len(c.markers))
        h2 = Heal(par, c, preset=c.preset)
        dev2 = h2.inpaint([c.markers[k] for k in order])
        assert np.array_equal(bits(dev), bits(dev2))
        assert h2.mask.guards_intact() and h2.spec.unchanged()
    assert h.mask.guards_intact() and h.spec.unchanged()


def test_inpaint_mask_sweep(par):
    worst = cells = same = 0
    for seed in H.SWEEP_SEEDS:
        c = H.sweep_case(seed)
        h = Heal(par, c)
        dev = h.inpaint()
        w, n, e = check_mask(c, dev, H.gain_mask_np(c.spec, c.markers))
        worst, cells, same = max(worst, w), cells + n, same + e
        dev2 = Heal(par, c).inpaint(c.markers[::-1])
        assert np.array_equal(bits(dev), bits(dev2)), c
        assert h.mask.guards_intact() and h.spec.unchanged(), c
    print(f"\nsweep: worst |mask - float64| {worst:.2e} dB; {same} of {cells} box cells bit-equal to float32(ref)")


@pytest.mark.parametrize("kind", ["nan", "nan_neg", "inf"])
def test_inpaint_poison_values(par, kind):
    """np.clip keeps a NaN: a NaN in a surrounding frame of one bin makes that bin's box cells NaN, whichever way round the overlapping
    marker comes; an Inf gives [255, ..., 255, NaN].  (The reference's NaN in the NEXT LOWER bin is scipy's 0 * NaN in its
    interpolation along bins, which the kernel does not perform: not reproduced.)  The apply kernel then makes those bins NaN."""
    c, b = H.poison_case(kind)
    for ms in (c.markers, c.markers[::-1]):
        h = Heal(par, c)
        dev = h.inpaint(ms)
        ref = H.gain_mask_np(c.spec, ms)
        fb, fa = c.markers[0][:2]
        assert np.array_equal(np.isnan(dev[fb:fa, b]), np.isnan(ref[fb:fa, b])), (kind, dev[fb:fa, b], ref[fb:fa, b])
        assert np.isnan(ref).sum() == (1 if kind == "inf" else fa - fb)
        assert np.all(bits(dev[np.isnan(dev)]) >> 31 == 0)                       # a positive NaN: it wins the integer max
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(dev), ~fin)
        ref32 = ref.astype(np.float32)
        assert np.all(np.abs(dev[fin].astype(np.float64) - ref32[fin]) <= np.maximum(np.spacing(np.abs(ref32[fin])), 1e-9))
        assert np.array_equal(dev[fin] > 0, ref[fin] > 0)
        out = h.apply(ms)
        want = H.apply_np(c.spec, dev)
        poisoned = ~np.isfinite(want)
        assert poisoned.sum() >= np.isnan(dev).sum() and np.all(np.isnan(out[np.isnan(dev)]))
        ok = ~poisoned
        assert np.all(np.abs(out[ok] - want[ok]) <= TOL * np.abs(want[ok]))
        assert not h.mask.read().any() and h.mask.guards_intact() and h.spec.guards_intact()


# ------------------------------------------------------------------------------------------ apply
APPLY_WORST = {"err": 0.0}


def run_apply(par, c):
    h = Heal(par, c, preset=c.preset)
    mask = h.inpaint()
    out = h.apply()
    inside = H.box_cells(mask.shape, c.markers)
    want = H.apply_np(c.spec, np.where(inside, mask, np.float32(0)))      # the boxes only: a pre-set value outside them is not the call's
    assert out.dtype == np.complex64 and out.shape == want.shape
    err = np.abs(out.astype(np.complex128) - want)
    bad = np.argwhere(~(err <= TOL * np.abs(want)))
    assert len(bad) == 0, (c, len(bad), bad[:5].tolist())
    assert np.array_equal(bits(out[~inside]), bits(np.asarray(c.spec)[~inside])), c        # outside the boxes: the input's bits
    assert np.array_equal(bits(out[mask == 0]), bits(np.asarray(c.spec)[mask == 0])), c    # a zero gain: untouched
    after = h.mask.read()
    assert np.array_equal(bits(after), bits(np.where(inside, np.float32(0), mask))), c     # cleared over the boxes (all zeros without a preset)
    nz = np.abs(want) > 0
    rel = np.zeros(err.shape)
    rel[nz] = err[nz] / np.abs(want[nz])
    k = np.unravel_index(np.argmax(rel), rel.shape)
    if rel[k] > APPLY_WORST["err"]:
        APPLY_WORST.update(err=float(rel[k]), gain=float(mask[k]), case=c.name)
    if c.preset is None:
        assert not after.any()
        # the same mask buffer again, a fresh copy of the spectrogram: the identical result
        h.new_spec()
        mask2 = h.inpaint()
        out2 = h.apply()
        assert np.array_equal(bits(mask2), bits(mask)) and np.array_equal(bits(out2), bits(out)), c
        assert not h.mask.read().any()
    assert h.mask.guards_intact() and h.spec.guards_intact(), c
    return float(rel[k]), float(mask[k])


@pytest.mark.parametrize("name", H.NAMED)
def test_apply_named(par, name):
    c = H.case(name)
    g = H.kernel_geometry([m for m in c.markers if H.marker_valid(m, c.frames, c.bins)][0])
    if "apply_loops" in c.expect:
        assert g["apply_loops"] == c.expect["apply_loops"]         # nb >= 256: the bi += 256 loop; below: the lane form
    rel, gain = run_apply(par, c)
    print(f"\n{name}: worst per-bin error {rel:.2e} of the bin's magnitude, at a gain of {gain:.3f} dB")


def test_apply_sweep(par):
    for seed in H.SWEEP_SEEDS:
        run_apply(par, H.sweep_case(seed))
    print(f"\napply, named cases and sweep: worst per-bin error {APPLY_WORST['err']:.3e} at a gain of {APPLY_WORST.get('gain', 0):.3f} dB "
          f"({APPLY_WORST.get('case')})")


# ------------------------------------------------------------------------------------------ band mean
def band_mean(par, mag, bins, bl, bu, fb, fa, pitched):
    frames = mag.shape[0]
    body = mag
    if pitched:
        body = np.full((frames, bins + 37), np.float32(3e38))
        body[:, :bins] = mag
    m = Guarded(par, body, 2, np.float32(3e38))
    out = Guarded(par, np.full(fa - fb, -1234.5), 8, -1234.5)
    par.check(par.L.par_band_mean_db_f32(par.dev, m.ptr(), frames, bins, body.shape[1] if pitched else 0, bl, bu, fb, fa, out.ptr(),
                                         par.stream()))
    got = out.read().copy()
    assert out.guards_intact() and m.unchanged()
    return got


@pytest.mark.parametrize("bins,band", [(300, (5, 6)), (300, (3, 66)), (300, (3, 67)), (300, (3, 68)), (300, (236, 300)), (1025, (0, 1025))])
def test_band_mean_db(par, bins, band):
    mag = H.band_mag(bins + band[0], 9, bins)
    worst = 0.0
    for fb, count in ((0, 9), (2, 1), (2, 3), (2, 4), (2, 5), (8, 1)):
        for pitched in (False, True):
            got = band_mean(par, mag, bins, band[0], band[1], fb, fb + count, pitched)
            ref = H.band_mean_db_np(mag, band[0], band[1], fb, fb + count)
            worst = max(worst, float(np.max(np.abs(got - ref))))
    print(f"\nband mean over {band[1] - band[0]} bins: worst {worst:.2e} dB")
    assert worst <= BAND_TOL


def test_band_mean_db_special_values(par):
    mag = H.band_mag(3, 6, 70).copy()
    mag[1, 5], mag[2, 6], mag[3, 7] = 0.0, np.nan, np.float32(1e-40)
    for bl, bu in ((0, 70), (5, 8)):
        got = band_mean(par, mag, 70, bl, bu, 0, 6, True)
        with np.errstate(all="ignore"):
            ref = H.band_mean_db_np(mag, bl, bu, 0, 6)
        assert got[1] == -np.inf == ref[1] and np.isnan(got[2]) and np.isnan(ref[2])
        fin = [0, 3, 4, 5]
        assert np.isfinite(got[fin]).all() and np.max(np.abs(got[fin] - ref[fin])) <= BAND_TOL


# ------------------------------------------------------------------------------------------ curve scale, accumulate
@pytest.mark.parametrize("n,frames", H.CURVE_SHAPES)
def test_curve_scale(par, n, frames):
    worst, total, same = 0.0, 0, 0
    for n_ch, stride in H.CHANNELS:
        sig, fac = H.curve_case(n, frames, n_ch, stride)
        s = Guarded(par, sig, 4, np.float32(7e37))
        f = Guarded(par, fac, 2, 1e300)
        out = Guarded(par, np.full(n_ch * n, -1234.5), 64, -1234.5)
        par.check(par.L.par_curve_scale_f64(par.dev, s.ptr(), stride, n_ch, n, f.ptr(), frames, out.ptr(), par.stream()))
        got = out.read().reshape(n_ch, n).copy()
        ref, bound = H.curve_scale_np(sig, fac), H.curve_scale_bound(sig, fac)
        err = np.abs(got - ref)
        bad = np.argwhere(~(err <= bound))
        assert len(bad) == 0, (n, frames, n_ch, stride, bad[:5].tolist())
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        total, same = total + got.size, same + int(np.sum(bits(got) == bits(ref)))
        assert out.guards_intact() and s.unchanged() and f.unchanged()
    print(f"\ncurve scale ({n}, {frames}): worst error {worst:.3f} of the bound; {same} of {total} outputs bit-equal to numpy")


@pytest.mark.parametrize("n", [1, 2, 13, 255, 256, 257, 100001])
def test_accumulate(par, n):
    for n_ch, stride in H.CHANNELS:
        sig, y = H.accumulate_case(n, n_ch, stride)
        s = Guarded(par, sig, 4, np.float32(7e37))
        yy = Guarded(par, y.reshape(-1), 64, 1e300)
        par.check(par.L.par_accumulate_f64_f32(par.dev, s.ptr(), stride, n_ch, n, yy.ptr(), par.stream()))
        got = s.read()
        assert np.array_equal(bits(got), bits(H.accumulate_np(sig, y))), (n, n_ch, stride)      # the stride's spare columns included
        assert s.guards_intact() and yy.unchanged()


# ------------------------------------------------------------------------------------------ copy segments
OTHER = np.float32(9e37)


@pytest.mark.parametrize("strides", [(1, 1), (2, 2), (2, 1), (1, 3)])
@pytest.mark.parametrize("name", H.COPY_CASES)
def test_copy_segments(par, name, strides):
    c = H.copy_case(name)
    ss, ds = strides
    src = np.full((len(c.src), ss), OTHER, dtype=np.float32)
    src[:, ss - 1] = c.src                                         # the last channel of an interleaved file
    s = Guarded(par, src, 128, OTHER)
    d = Guarded(par, np.full((c.dst_len, ds), H.SENTINEL, dtype=np.float32), 128, H.SENTINEL)
    idx = dev_i(par, np.stack((c.src_start, c.dst_start, c.lens, c.run_start)), np.int64)
    p = [ctypes.c_void_p(idx[k].data_ptr()) for k in range(4)]
    par.check(par.L.par_copy_segments_f32(par.dev, s.ptr(ss - 1), ss, c.n_valid, c.n_padded, int(c.padded), p[0], p[1], p[2], p[3],
                                          len(c.lens), c.total, d.ptr(ds - 1), ds, par.stream()))
    got = d.read()
    want = np.full((c.dst_len, ds), H.SENTINEL, dtype=np.float32)
    want[:, ds - 1] = H.copy_segments_np(c)
    assert np.array_equal(bits(got), bits(want)), (name, np.argwhere(bits(got) != bits(want))[:5].tolist())
    assert d.guards_intact() and s.unchanged()


# ------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(par):
    """PAR_ERR_ARG (1) before any launch: the non-null pointers are never followed"""
    L, dev, p = par.L, par.dev, ctypes.c_void_p(8)
    for fn in (L.par_inpaint_gain_db_c64, L.par_spec_apply_gain_boxes_c64):
        assert fn(dev, None, 10, 10, p, 1, p, None) == 1
        assert fn(dev, p, 10, 10, None, 1, p, None) == 1
        assert fn(dev, p, 10, 10, p, 1, None, None) == 1
        assert fn(dev, p, 0, 10, p, 1, p, None) == 1
        assert fn(dev, p, 10, 0, p, 1, p, None) == 1
        assert fn(dev, p, 10, 10, p, -1, p, None) == 1
        assert fn(dev, p, 10, 10, p, 0, p, None) == 0                                  # no markers: nothing to do
    bm = L.par_band_mean_db_f32
    assert bm(dev, None, 10, 10, 0, 1, 5, 0, 10, p, None) == 1
    assert bm(dev, p, 10, 10, 0, 1, 5, 0, 10, None, None) == 1
    assert bm(dev, p, 10, 10, 0, 5, 5, 0, 10, p, None) == 1                            # empty band
    assert bm(dev, p, 10, 10, 0, 6, 5, 0, 10, p, None) == 1
    assert bm(dev, p, 10, 10, 0, -1, 5, 0, 10, p, None) == 1
    assert bm(dev, p, 10, 10, 0, 1, 11, 0, 10, p, None) == 1                           # past the last bin
    assert bm(dev, p, 10, 10, 0, 1, 5, 0, 11, p, None) == 1                            # frame_a > n_frames
    assert bm(dev, p, 10, 10, 0, 1, 5, 6, 5, p, None) == 1
    assert bm(dev, p, 10, 10, 9, 1, 5, 0, 10, p, None) == 1                            # pitch < bins
    assert bm(dev, p, 10, 10, 0, 1, 5, 4, 4, p, None) == 0                             # no frames: nothing to do
    cs = L.par_curve_scale_f64
    assert cs(dev, None, 1, 1, 10, p, 3, p, None) == 1 and cs(dev, p, 1, 1, 10, None, 3, p, None) == 1
    assert cs(dev, p, 1, 1, 10, p, 3, None, None) == 1
    assert cs(dev, p, 1, 0, 10, p, 3, p, None) == 1                                    # n_ch = 0
    assert cs(dev, p, 1, 2, 10, p, 3, p, None) == 1                                    # sig_stride < n_ch
    assert cs(dev, p, 1, 1, 0, p, 3, p, None) == 1 and cs(dev, p, 1, 1, 10, p, 0, p, None) == 1
    ac = L.par_accumulate_f64_f32
    assert ac(dev, None, 1, 1, 10, p, None) == 1 and ac(dev, p, 1, 1, 10, None, None) == 1
    assert ac(dev, p, 1, 0, 10, p, None) == 1 and ac(dev, p, 1, 2, 10, p, None) == 1 and ac(dev, p, 1, 1, 0, p, None) == 1
    cp = L.par_copy_segments_f32
    good = [dev, p, 1, 5, 5, 0, p, p, p, p, 1, 5, p, 1, None]
    for k in (1, 6, 7, 8, 9, 12):
        a = list(good)
        a[k] = None
        assert cp(*a) == 1, k
    for k, v in ((2, 0), (13, 0), (10, -1), (11, -1)):                                  # src_stride = 0, dst_stride = 0, negative sizes
        a = list(good)
        a[k] = v
        assert cp(*a) == 1, k
    a = list(good)
    a[4], a[5] = 0, 1                                                                   # padded with n_padded = 0
    assert cp(*a) == 1
    a = list(good)
    a[10] = 0
    assert cp(*a) == 0                                                                  # no segments: nothing to do
