"""Which K_sinc a file gets (csrc/sinc_route.h: the block kernel, or the streaming kernel in its mono, one-channel-of-two or stereo
form), pinned at the sizes where the rule changes its answer: 4096 outputs and 4096 input samples, where the large files of
tests/test_hip_parity.py do not reach.  Inputs and their preconditions: tests/sinc_route_inputs.py, test_sinc_route_inputs_cpu.py.

Every result is held to the C oracle at the TOL of tests/test_hip_parity.py.  The two kernels differ by float32 rounding, which is
how test_kernel_choice_of_the_fused_entry_point tells them apart and how these tests do: a file the rule sends to the block
kernel comes out BIT-equal to the same call under par_debug_sinc_kernel(0); a file it sends to the streaming kernel agrees with
that call within that test's 5e-6 and is not bit-equal to it (at four tiles the streams take tile 1 only: 1024 outputs).  The
batch entry point is driven directly through _lib.FusedItem -- the Python driver never sends it a mixed group -- and every
output must be bit-equal to the same item through par_varispeed_fused_f32 / _stereo_f32."""
import numpy as np
import pytest

import sinc_route_inputs as I
from test_hip_parity import TOL, par, relerr, sinc_kernel  # noqa: F401  (par, sinc_kernel: the fixtures)

pytestmark = pytest.mark.gpu

KERNELS_APART = 5e-6          # test_kernel_choice_of_the_fused_entry_point


class Ctx:
    """plans (one per curve name: a batch uses a name once, every item its own work / aux) and oracle positions, made once"""

    def __init__(self, par):
        self.par, self.t = par, par.torch
        self._plans, self._pos, self._want = {}, {}, {}

    def plan(self, name):
        if name not in self._plans:
            t = self.t
            st, sp = I.speed_curve(name)
            plan = self.par.resampling.speed_plan_dev(t.from_numpy(st).cuda(), t.from_numpy(sp).cuda(), I.CURVES[name].n_in, fused=True)
            assert plan.fused_ok and plan.len_out == I.CURVES[name].len_out, (name, plan.len_out)
            self._plans[name] = plan
        return self._plans[name]

    def want(self, name, key, col, NT):
        from oracle import oracle_c as C
        if name not in self._pos:
            st, sp = I.speed_curve(name)
            self._pos[name] = C.speed_to_pos(st, sp, I.CURVES[name].n_in)[0]
        if (name, key, NT) not in self._want:
            self._want[name, key, NT] = C.sinc(self._pos[name], np.ascontiguousarray(col), NT)
        return self._want[name, key, NT]


@pytest.fixture(scope="module")
def ctx(par):
    return Ctx(par)


class Item:
    """One file in one layout.  kind: "mono"; ("strided", sig_stride, out_stride): the last channel of sig_stride-channel frames,
    outputs out_stride apart; "stereo": both channels of an interleaved file into an interleaved output; "stereo_4mod8": the same
    with out0 at an address 4 mod 8; "stereo_planar_sig" / "stereo_planar_out": strides 2, but the second input / output
    channel lies in a buffer of its own (sig1 != sig0 + 1 / out1 != out0 + 1)."""

    def __init__(self, ctx, name, kind):
        t, c = ctx.t, I.CURVES[name]
        self.ctx, self.name, self.kind, self.plan, self.n_out, self.len_in = ctx, name, kind, ctx.plan(name), c.len_out, c.n_in

        def up(a):
            return t.from_numpy(np.ascontiguousarray(a)).cuda().reshape(-1)
        if kind == "mono" or kind[0] == "strided":
            ss, so = (1, 1) if kind == "mono" else kind[1:]
            x = I.signal(name, ss) if ss > 1 else I.signal(name)[:, None]
            self.sig0, self.sig1, self.sig_stride, self.out_stride = up(x)[ss - 1:], None, ss, so
            self.cols = [x[:, ss - 1]]
        else:
            x = I.signal(name, 2)
            flat = up(x)
            self.sig0, self.sig1, self.sig_stride, self.out_stride = flat[0:], flat[1:], 2, 2
            self.cols = [x[:, 0], x[:, 1]]
            if kind == "stereo_planar_sig":
                y = I.signal(name, 2, seed=1)
                self.sig1, self.cols[1] = up(y)[0:], y[:, 0]

    def outputs(self):
        """fresh output buffers holding 7.0 -> (out0, out1, read); read() -> the result, (n_out,) or (n_out, 2), after checking
        that nothing beside it was written"""
        t, n, so = self.ctx.t, self.n_out, self.out_stride

        def full(k):
            return t.full((k,), 7.0, dtype=t.float32, device="cuda")
        if self.sig1 is None:
            buf = full(n * so)

            def read():
                a = buf.cpu().numpy().reshape(n, so)
                assert np.all(a[:, 1:] == 7.0)
                return a[:, 0].copy()
            return buf, None, read
        if self.kind == "stereo_planar_out":
            a, b = full(2 * n), full(2 * n)

            def read():
                A, B = a.cpu().numpy().reshape(n, 2), b.cpu().numpy().reshape(n, 2)
                assert np.all(A[:, 1] == 7.0) and np.all(B[:, 1] == 7.0)
                return np.stack((A[:, 0], B[:, 0]), axis=1)
            return a, b, read
        off = 1 if self.kind == "stereo_4mod8" else 0
        buf = full(2 * n + off)
        assert buf[off:].data_ptr() % 8 == 4 * off

        def read():
            a = buf.cpu().numpy()
            assert np.all(a[:off] == 7.0)
            return a[off:].reshape(n, 2).copy()
        return buf[off:], buf[off + 1:], read

    def single(self, NT=32):
        """through par_varispeed_fused_f32 / par_varispeed_fused_stereo_f32"""
        R = self.ctx.par.resampling
        out0, out1, read = self.outputs()
        lay = dict(sig_stride=self.sig_stride, len_in=self.len_in, out_stride=self.out_stride)
        if self.sig1 is None:
            R.varispeed_fused_dev(self.plan, self.sig0, NT, out0, **lay)
        else:
            R.varispeed_fused_stereo_dev(self.plan, self.sig0, self.sig1, NT, out0, out1, **lay)
        return read()

    def check_oracle(self, got, NT=32):
        for c, col in enumerate(self.cols):
            want = self.ctx.want(self.name, (self.kind, c), col, NT)
            g = got if got.ndim == 1 else got[:, c]
            assert relerr(g, want) < TOL, (self.name, self.kind, NT, c, relerr(g, want))


def run_batch(ctx, items, NT=32):
    """par_varispeed_fused_batch_f32 on the items, each into fresh buffers -> their results"""
    from pyaudiorestoration_amd import _lib, _dev
    arr = (_lib.FusedItem * len(items))()
    reads, keep = [], []
    for f, it in zip(arr, items):
        out0, out1, read = it.outputs()
        keep.append((out0, out1))
        reads.append(read)
        p = it.plan
        f.speeds, f.m, f.work, f.aux = p.speeds_t.data_ptr(), p.m, p.work.data_ptr(), p.aux.data_ptr()
        f.max_out, f.len_out = p.max_out, p.len_out
        f.sig0, f.sig1 = it.sig0.data_ptr(), (it.sig1.data_ptr() if it.sig1 is not None else None)
        f.out0, f.out1 = out0.data_ptr(), (out1.data_ptr() if out1 is not None else None)
        f.sig_stride, f.len_in, f.out_stride = it.sig_stride, it.len_in, it.out_stride
    _lib.check(_lib.lib().par_varispeed_fused_batch_f32(0, len(items), arr, int(NT), _dev.stream_ptr(0)))
    return [r() for r in reads]


BLOCK_CASES = [
    ("below", "mono", 32),                       # 4095 outputs
    ("short_in", "mono", 32),                    # 4095 input samples
    ("edge", "mono", 50),
    ("edge", "mono", 16),
    ("edge", ("strided", 3, 1), 32),             # a channel of a three-channel file
    ("edge", ("strided", 1, 2), 32),             # unit input, outputs two apart
    ("below", ("strided", 2, 1), 32),
    ("short_in", ("strided", 2, 2), 32),
    ("edge", "stereo_4mod8", 32),
    ("edge", "stereo_planar_sig", 32),
    ("edge", "stereo_planar_out", 32),
    ("edge", "stereo", 50),
    ("below", "stereo", 32),
    ("short_in", "stereo", 32),
]
STREAM_CASES = [
    ("edge", "mono"),                            # 4096 outputs
    ("edge_in", "mono"),                         # 4096 input samples
    ("edge", ("strided", 2, 1)),
    ("edge", ("strided", 2, 2)),
    ("edge", ("strided", 2, 3)),
    ("edge", "stereo"),
    ("f4", "stereo"),                            # six tiles and a partial one
]
# (not among them: "edge_in" as a stereo file or as one channel of two.  On its 5 % fast curve the streams hand tile 1 to the
# tile list -- par_fused_redo_tiles reads 1 -- and those two forms do a file's end tiles with the block kernel's own code, so
# their output is the block kernel's bit for bit whichever route ran.  The mono form's end tiles round differently: it stays.)


def _id(case):
    return "-".join("x".join(str(v) for v in p) if isinstance(p, tuple) else str(p) for p in case)


@pytest.mark.parametrize("case", BLOCK_CASES, ids=_id)
def test_block_route(ctx, sinc_kernel, case):
    name, kind, NT = case
    it = Item(ctx, name, kind)
    got = it.single(NT)
    sinc_kernel(0)
    forced = it.single(NT)
    it.check_oracle(got, NT)
    assert np.array_equal(got, forced)


@pytest.mark.parametrize("case", STREAM_CASES, ids=_id)
def test_stream_route(ctx, sinc_kernel, case):
    name, kind = case
    it = Item(ctx, name, kind)
    got = it.single()
    sinc_kernel(0)
    forced = it.single()
    it.check_oracle(got)
    it.check_oracle(forced)
    print(f"{_id(case)}: default against forced block kernel {relerr(got, forced):.3e}, differing outputs {int(np.sum(got != forced))}")
    assert relerr(got, forced) < KERNELS_APART and not np.array_equal(got, forced)


BATCH_CASES = {
    "one": [("edge", "mono")],
    "two_mono": [("edge", "mono"), ("f3", "mono")],
    "two_stereo": [("edge", "stereo"), ("f4", "stereo")],
    "mono_and_stereo": [("f1", "mono"), ("f2", "stereo")],
    "one_below_the_edge": [("edge", "mono"), ("below", "mono"), ("f5", "mono")],
    "one_channel_of_two_among_mono": [("f1", "mono"), ("f6", ("strided", 2, 1)), ("f7", "mono")],
    "one_stereo_at_4mod8": [("f3", "stereo"), ("f8", "stereo_4mod8"), ("edge", "stereo")],
    "nine_mono": [(n, "mono") for n in I.MONO_NINE],         # two launches, the second with one file
    "two_mono_block_kernel_forced": [("f2", "mono"), ("f4", "mono")],
}


@pytest.mark.parametrize("case", sorted(BATCH_CASES))
def test_batch_equals_item_by_item(ctx, sinc_kernel, case):
    items = [Item(ctx, name, kind) for name, kind in BATCH_CASES[case]]
    if case.endswith("forced"):
        sinc_kernel(0)
    got = run_batch(ctx, items)
    for it, g in zip(items, got):
        it.check_oracle(g)
        assert np.array_equal(g, it.single()), (case, it.name, it.kind)
