"""The spectrogram image kernels at the ABI.  The expected image is np.max over the cells (tests/spectrogram_np.py) of the array
par_stft_f32 mode 1 stored for the same call; par_stft_peak_image_f32 (fused) and par_peak_image_f32 (composed) must equal it
bit for bit, compared as uint32.  Every call writes into a pitched image (pitch = height + 3) laid between guards, with a
sentinel in the cells between the columns, and into a scratch laid between guards; all of them must survive."""
import ctypes

import numpy as np
import pytest
import scipy.signal

import spectrogram_np as SN

pytestmark = pytest.mark.gpu

SENT = 0x7B7B7B7B
GUARD = 64


@pytest.fixture(scope="module")
def env():
    import torch
    from pyaudiorestoration_amd import _dev, _lib, spectrogram
    assert torch.cuda.is_available()

    class E:
        pass
    e = E()
    e.torch, e.dev, e.lib, e.L, e.sp = torch, _dev, _lib, _lib.lib(), spectrogram
    return e


def noise(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


class Case:
    """One signal on the device with its stored mode-1 spectrogram"""

    def __init__(self, env, x, n_fft, hop, zeropad=1, stride=1, window="blackmanharris", offset=0):
        T = env.torch
        self.env, self.n_fft, self.hop, self.zp, self.stride = env, n_fft, hop, zeropad, stride
        self.n = len(x)
        buf = np.full(self.n * stride, 7.0, dtype=np.float32)          # the other channels hold a constant nobody may read into the picture
        buf[offset::stride] = x
        self.x_t = T.from_numpy(buf).cuda()
        self.x_ptr = ctypes.c_void_p(self.x_t.data_ptr() + 4 * offset)
        self.win_t = T.from_numpy(scipy.signal.get_window(window, n_fft).astype(np.float32)).cuda()
        self.bins = n_fft * zeropad // 2 + 1
        self.frames = int(env.L.par_stft_frames(self.n, n_fft, hop))
        M = n_fft * zeropad
        self.mag_t = T.empty((self.frames, self.bins), dtype=T.float32, device="cuda")
        if M <= 16384:
            env.lib.check(env.L.par_stft_f32(0, self.x_ptr, self.n, stride, n_fft, hop, zeropad, env.dev.ptr(self.win_t),
                                             env.dev.ptr(self.mag_t), 1, self.bins, None))
        else:
            nbytes = int(env.L.par_stft_big_scratch_bytes(self.n, n_fft, hop, zeropad))
            scratch = T.empty(nbytes, dtype=T.uint8, device="cuda")
            env.lib.check(env.L.par_stft_big_f32(0, self.x_ptr, self.n, stride, n_fft, hop, zeropad, env.dev.ptr(self.win_t),
                                                 env.dev.ptr(self.mag_t), 1, env.dev.ptr(scratch), nbytes, None))
        self.mag = self.mag_t.cpu().numpy()

    def image_buffer(self, width, height, pitch, zero_cells):
        T = self.env.torch
        buf = T.full((GUARD + width * pitch + GUARD,), SENT, dtype=T.int32, device="cuda")
        if zero_cells:
            buf[GUARD:GUARD + width * pitch].view(width, pitch)[:, :height] = 0
        return buf

    @staticmethod
    def split(buf, width, height, pitch):
        """-> (cells uint32 (width, height), everything else uint32)"""
        a = buf.cpu().numpy().view(np.uint32)
        body = a[GUARD:GUARD + width * pitch].reshape(width, pitch)
        rest = np.concatenate([a[:GUARD], body[:, height:].ravel(), a[GUARD + width * pitch:]])
        return body[:, :height].copy(), rest

    def tables(self, cols, rows):
        T = self.env.torch
        cols = np.ascontiguousarray(cols, dtype=np.int64)
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        return cols, rows, T.from_numpy(cols).cuda(), T.from_numpy(rows).cuda()

    def fused(self, cols, rows, extra=3):
        env, T = self.env, self.env.torch
        cols, rows, cols_t, rows_t = self.tables(cols, rows)
        width, height = len(cols), len(rows)
        pitch = height + extra
        buf = self.image_buffer(width, height, pitch, zero_cells=False)
        need = int(env.L.par_stft_peak_image_scratch_bytes(width))
        assert need == 8 * (width + 1)
        scratch = T.full((GUARD * 4 + need + GUARD * 4,), 0xA5, dtype=T.uint8, device="cuda")
        env.lib.check(env.L.par_stft_peak_image_f32(0, self.x_ptr, self.n, self.stride, self.n_fft, self.hop, self.zp, env.dev.ptr(self.win_t),
                                                    env.dev.ptr(cols_t), cols.ctypes.data, env.dev.ptr(rows_t), rows.ctypes.data, width, height,
                                                    ctypes.c_void_p(buf.data_ptr() + 4 * GUARD), pitch,
                                                    ctypes.c_void_p(scratch.data_ptr() + 4 * GUARD), need, None))
        cells, rest = self.split(buf, width, height, pitch)
        assert np.all(rest == SENT), "the fused call wrote outside the image's cells"
        s = scratch.cpu().numpy()
        assert np.all(s[:4 * GUARD] == 0xA5) and np.all(s[4 * GUARD + need:] == 0xA5), "the fused call wrote outside its scratch"
        return cells

    def composed(self, cols, rows, seams=(), extra=3, order=None):
        """the stored spectrogram handed over in chunks cut at `seams` (frame numbers), in `order`"""
        env = self.env
        cols, rows, cols_t, rows_t = self.tables(cols, rows)
        width, height = len(cols), len(rows)
        pitch = height + extra
        buf = self.image_buffer(width, height, pitch, zero_cells=True)
        edges = [0] + sorted(seams) + [self.frames]
        chunks = list(zip(edges[:-1], edges[1:]))
        for k in (order if order is not None else range(len(chunks))):
            fa, fb = chunks[k]
            env.lib.check(env.L.par_peak_image_f32(0, ctypes.c_void_p(self.mag_t.data_ptr() + 4 * fa * self.bins), self.bins, self.bins,
                                                   self.frames, fa, fb - fa, env.dev.ptr(cols_t), cols.ctypes.data, env.dev.ptr(rows_t),
                                                   rows.ctypes.data, width, height, ctypes.c_void_p(buf.data_ptr() + 4 * GUARD), pitch, None))
        cells, rest = self.split(buf, width, height, pitch)
        assert np.all(rest == SENT), "the composed call wrote outside the image's cells"
        return cells

    def expected(self, cols, rows):
        cols, rows = np.asarray(cols), np.asarray(rows)
        return SN.peak_tables_np(self.mag, cols[:, 0], cols[:, 1], rows[:, 0], rows[:, 1])

    def check(self, cols, rows, what, seams=None, fused=True):
        want = self.expected(cols, rows).view(np.uint32)
        if fused:
            got = self.fused(cols, rows)
            assert np.array_equal(got, want), (what, "fused", int((got != want).sum()), got.shape)
        seams = seams if seams is not None else [self.frames // 3, self.frames // 3 + 1, 2 * self.frames // 3]
        got = self.composed(cols, rows, [s for s in seams if 0 < s < self.frames])
        assert np.array_equal(got, want), (what, "composed", int((got != want).sum()), got.shape)
        return want

    def geometry(self, width, height, sr=8000.0, **kw):
        return self.env.sp.geometry(self.n, sr, self.n_fft, self.hop, self.zp, width, height, **kw)


def n_for(frames, hop):
    return (frames - 1) * hop + 1


# -------------------------------------------------------------------------------------------------------- every compiled size
@pytest.mark.parametrize("log_m", range(4, 15))
def test_every_transform_size_once(env, log_m):
    n_fft = 1 << log_m
    hop = max(1, n_fft // 4)
    c = Case(env, noise(n_for(24, hop), log_m), n_fft, hop)
    g = c.geometry(7, 5)
    c.check(*g.tables(), what=n_fft)
    g = c.geometry(c.frames, min(c.bins, 40), scale="linear")               # one frame per column: nothing may hide in a maximum
    c.check(*g.tables(), what=(n_fft, "1:1"))


# ---------------------------------------------------------------------------------------------------------- the detailed cases
DETAIL = [64, 512, 2048, 16384]


@pytest.mark.parametrize("n_fft", DETAIL)
def test_widths_heights_and_scales(env, n_fft):
    hop = n_fft // 4
    frames = 60 if n_fft < 16384 else 36
    c = Case(env, noise(n_for(frames, hop), 100 + n_fft), n_fft, hop)
    assert c.frames == frames
    heights = [1, 7, c.bins, 2 * c.bins]
    scales = [dict(scale="mel"), dict(scale="linear"), dict(scale="log", f0=30.0)]
    for i, width in enumerate([1, 3, frames - 1, frames, frames + 1, 3 * frames]):
        g = c.geometry(width, heights[i % 4], **scales[i % 3])
        if width == 1:
            assert g.col_hi[0] - g.col_lo[0] == frames and -(-frames // 16) >= 3   # chunks of at most 16 frames: three or more of them
        c.check(*g.tables(), what=(n_fft, width, heights[i % 4], scales[i % 3]))
    for j, height in enumerate(heights):                                     # every height in every scale at one width
        for k, kw in enumerate(scales):
            if (j + k) % 2 == 0 or n_fft == 64:
                g = c.geometry(11, height, **kw)
                c.check(*g.tables(), what=(n_fft, 11, height, kw))


@pytest.mark.parametrize("n_fft", DETAIL)
def test_empty_columns_and_row_orders(env, n_fft):
    hop = n_fft // 4
    c = Case(env, noise(n_for(40, hop), 200 + n_fft), n_fft, hop)
    dur = c.frames * hop / 8000.0
    for width in (9, 50, 170):
        g = c.geometry(width, 9, t0=-0.4 * dur, t1=1.5 * dur)
        assert g.col_hi[0] == g.col_lo[0] == 0 and g.col_hi[-1] == g.col_lo[-1] == c.frames
        want = c.check(*g.tables(), what=(n_fft, width, "empty sides"))
        assert not want[0].any() and not want[-1].any() and want[width // 2].all()
    g = c.geometry(6, 12, f0=100.0)
    cols, rows = g.tables()
    want = c.check(cols, rows, what="top first").view(np.float32)
    up = c.check(cols, rows[::-1], what="ascending rows").view(np.float32)
    assert np.array_equal(up[:, ::-1].view(np.uint32), want.view(np.uint32))
    perm = np.random.default_rng(3).permutation(len(rows))
    mixed = np.concatenate([rows[perm], [[0, 0], [c.bins, c.bins], [0, 5]]])        # arbitrary order, empty rows, an overlapping row
    got = c.check(cols, mixed, what="mixed rows").view(np.float32)
    assert np.array_equal(got[:, :len(perm)].view(np.uint32), want[:, perm].view(np.uint32))
    assert not got[:, len(perm)].any() and not got[:, len(perm) + 1].any()
    # columns with gaps and repeats that no geometry makes
    cols = [[0, 0], [2, 3], [2, 3], [5, 26], [26, 26], [30, c.frames], [30, c.frames], [c.frames, c.frames]]
    c.check(cols, rows, what="gaps and repeats")


@pytest.mark.parametrize("n_fft", DETAIL)
def test_hops_strides_zero_padding_and_short_signals(env, n_fft):
    rng_seed = 300 + n_fft
    big = n_fft == 16384
    # hop > n_fft, and an odd hop
    for hop in (n_fft + 3, n_fft // 4 + 1):
        c = Case(env, noise(n_for(21, hop), rng_seed + hop % 7), n_fft, hop)
        g = c.geometry(5, 7)
        c.check(*g.tables(), what=(n_fft, "hop", hop))
    # a signal shorter than n_fft / 2: the reflection repeats
    n = max(3, n_fft // 2 - 5) if not big else n_fft // 2 - 5
    hop = max(1, n // 20)
    c = Case(env, noise(n, rng_seed + 1), n_fft, hop)
    assert 20 <= c.frames <= 60 or n_fft == 64
    g = c.geometry(4, 9)
    c.check(*g.tables(), what=(n_fft, "short"))
    g = c.geometry(c.frames, 5, scale="linear")
    c.check(*g.tables(), what=(n_fft, "short 1:1"))
    # zero padding 2 at the same transform size
    half = n_fft // 2
    c = Case(env, noise(n_for(24, half // 2), rng_seed + 2), half, half // 2, zeropad=2)
    assert c.bins == n_fft // 2 + 1
    g = c.geometry(5, 13)
    c.check(*g.tables(), what=(n_fft, "zeropad 2"))
    g = c.geometry(c.frames + 1, 6)
    c.check(*g.tables(), what=(n_fft, "zeropad 2 magnified"))
    # channel views of interleaved signals
    for stride, offset in ((2, 1), (3, 2)):
        hop = n_fft // 2
        c = Case(env, noise(n_for(22, hop), rng_seed + stride), n_fft, hop, stride=stride, offset=offset)
        g = c.geometry(6, 8)
        c.check(*g.tables(), what=(n_fft, "stride", stride))


@pytest.mark.parametrize("n_fft", DETAIL)
def test_impulse_halves_and_nan(env, n_fft):
    hop = n_fft // 4
    frames = 40
    n = n_for(frames, hop)
    # a unit impulse in silence: one hot stretch of frames among quiet ones
    x = np.zeros(n, dtype=np.float32)
    x[n // 2 + 1] = 1.0
    c = Case(env, x, n_fft, hop)
    for width in (1, 4, frames, frames + 7):
        g = c.geometry(width, 6)
        want = c.check(*g.tables(), what=(n_fft, "impulse", width)).view(np.float32)
        assert want.max() > 1e-4 and (width == 1 or want.min() == np.float32(1e-7))
    # loud / quiet halves
    x = noise(n, 400 + n_fft)
    x[: n // 2] *= 1e-4
    c = Case(env, x, n_fft, hop)
    for width in (2, 3, frames - 1):
        g = c.geometry(width, 5)
        c.check(*g.tables(), what=(n_fft, "halves", width))
    # one NaN sample: the cells whose frames cover it, and no others
    x = noise(n, 500 + n_fft)
    s = n // 2 + 3
    x[s] = np.nan
    c = Case(env, x, n_fft, hop)
    covering = [f for f in range(frames) if f * hop - n_fft // 2 <= s < f * hop - n_fft // 2 + n_fft]
    assert 3 <= len(covering) <= 5
    assert np.array_equal(np.flatnonzero(np.isnan(c.mag).any(axis=1)), covering) and np.isnan(c.mag[covering]).all()
    for width in (1, 5, frames, 2 * frames):
        g = c.geometry(width, 7)
        cols, rows = g.tables()
        want = c.expected(cols, rows)
        touched = np.array([any(a <= f < b for f in covering) for a, b in cols])
        assert np.array_equal(np.isnan(want), np.repeat(touched[:, None], 7, axis=1))
        for got in (c.fused(cols, rows), c.composed(cols, rows, [covering[1]])):
            got = got.view(np.float32)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (n_fft, width)
            ok = ~np.isnan(want)
            assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), (n_fft, width)


def test_composed_chunks_in_any_order_and_two_runs(env):
    n_fft, hop = 512, 128
    c = Case(env, noise(n_for(57, hop), 600), n_fft, hop)
    g = c.geometry(5, 9)
    cols, rows = g.tables()
    want = c.expected(cols, rows).view(np.uint32)
    assert any(a < s < b for a, b in cols for s in (7, 8, 30))               # the seams fall inside columns
    for seams, order in (([7, 8, 30], None), ([7, 8, 30], [3, 0, 2, 1]), (list(range(1, c.frames)), None), ([], None)):
        assert np.array_equal(c.composed(cols, rows, seams, order=order), want), seams
    first = c.fused(cols, rows)
    assert np.array_equal(first, want) and np.array_equal(c.fused(cols, rows), first)
    assert np.array_equal(c.fused(cols, rows, extra=0), want)                # pitch == height


def test_transform_above_the_fused_sizes(env):
    """2^15 points: four frames through par_stft_big_f32, the composed call on them; the fused call says UNSUPPORTED"""
    n_fft, hop = 1 << 15, 1 << 14
    c = Case(env, noise(3 * hop + 1, 700), n_fft, hop)
    assert c.frames == 4
    g = c.geometry(3, 11)
    cols, rows = g.tables()
    c.check(cols, rows, what="2^15", fused=False, seams=[1, 3])
    cols, rows, cols_t, rows_t = c.tables(cols, rows)
    T = env.torch
    peak = T.zeros((3, 11), dtype=T.float32, device="cuda")
    scratch = T.zeros(64, dtype=T.uint8, device="cuda")
    rc = env.L.par_stft_peak_image_f32(0, c.x_ptr, c.n, 1, n_fft, hop, 1, env.dev.ptr(c.win_t), env.dev.ptr(cols_t), cols.ctypes.data,
                                       env.dev.ptr(rows_t), rows.ctypes.data, 3, 11, env.dev.ptr(peak), 11, env.dev.ptr(scratch), 64, None)
    assert rc == 3 and not peak.any().item()


# ------------------------------------------------------------------------------------------------------------------- colours
def colour(env, peak, vmin, vmax, lut, extra=0):
    T = env.torch
    width, height = peak.shape
    pitch = height + extra
    buf = np.full((width, pitch), 123.0, dtype=np.float32)
    buf[:, :height] = peak
    peak_t = T.from_numpy(buf).cuda()
    lut_t = T.from_numpy(np.ascontiguousarray(lut, dtype=np.uint8)).cuda()
    out = T.full((GUARD + height * width + GUARD,), SENT, dtype=T.int32, device="cuda")
    env.lib.check(env.L.par_image_colorize_u8(0, env.dev.ptr(peak_t), width, height, pitch, vmin, vmax, env.dev.ptr(lut_t),
                                              ctypes.c_void_p(out.data_ptr() + 4 * GUARD), None))
    a = out.cpu().numpy()
    assert np.all(a[:GUARD] == SENT) and np.all(a[GUARD + height * width:] == SENT)
    return a[GUARD:GUARD + height * width].view(np.uint8).reshape(height, width, 4)


def identity_lut():
    i = np.arange(256, dtype=np.uint8)
    return np.stack([i, i, i, np.full(256, 255, dtype=np.uint8)], axis=1)


def test_colorize_step_centres_and_special_values(env):
    vmin, vmax = -120.0, 0.0
    t = np.arange(256) / 255.0
    centres = 10.0 ** ((vmin + t * (vmax - vmin)) / 20.0)
    special = [1e-7, 1e-9, 3.0, 1e30, 0.0, np.nan, np.float32(1e-6) * np.float32(1.0)]
    m = np.concatenate([centres, special]).astype(np.float32)
    peak = np.resize(m, (17, 31)).astype(np.float32)                        # every value several times, odd sides
    v = SN.colorize_t(peak, vmin, vmax)
    assert np.nanmin(np.abs(v - np.rint(v))) > 0.4                          # float32 keeps the centres well inside their steps
    for extra in (0, 5):
        got = colour(env, peak, vmin, vmax, identity_lut(), extra)
        want = SN.colorize_np(peak, vmin, vmax, identity_lut())
        assert np.array_equal(got, want)
    assert set(np.unique(want[..., 0])) == set(range(256))
    assert not got[peak.T == 0].any() and not got[np.isnan(peak.T)].any()


def test_colorize_random_magnitudes_and_a_real_table(env):
    m = SN.colorize_seeded_input()
    peak = m.reshape(128, 512)
    for vmin, vmax in ((-120.0, 0.0), (-96.3, -7.1)):
        got = colour(env, peak, vmin, vmax, identity_lut())
        want = SN.colorize_np(peak, vmin, vmax, identity_lut())
        diff = got[..., 0].astype(int) - want[..., 0].astype(int)
        v = SN.colorize_t(peak, vmin, vmax).T
        near = np.abs(v - np.rint(v)) < 1e-6
        assert np.all(diff[~near] == 0) and np.all(np.abs(diff) <= 1)
        assert np.all(got[..., 3] == 255) and np.array_equal(got[..., 0], got[..., 1])
    lut = np.random.default_rng(9).integers(0, 256, (256, 4), dtype=np.uint8)
    got = colour(env, peak, -120.0, 0.0, lut)
    idx = colour(env, peak, -120.0, 0.0, identity_lut())[..., 0]
    assert np.array_equal(got, lut[idx])                                    # the table passes through byte for byte
