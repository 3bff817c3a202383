"""The host-side rules of resampling.varispeed_batch_dev that need no device: work-item construction, look-ahead and ring size,
the planners / group options and the grouping step.  CPU tensors only."""
import types

import pytest
import torch

from pyaudiorestoration_amd import resampling as R

ST, SP = torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64)


def mono(n=10):
    return R.work_item((ST, SP, torch.zeros(n)))


def stereo(n=10):
    return R.work_item((ST, SP, torch.zeros(n, 2)))


def test_work_item_from_every_form_callers_pass():
    sig = torch.zeros(10)
    it = R.work_item((ST, SP, sig))
    assert it.st_t is ST and it.sp_t is SP and it.sig_t is sig
    assert (it.sig_stride, it.len_in, it.cls, it.n_samples) == (1, 10, "mono", 10)
    it = R.work_item((ST, SP, sig, 2))
    assert (it.sig_stride, it.len_in, it.cls) == (2, 5, None)
    it = R.work_item((ST, SP, sig, 2, 4))
    assert (it.sig_stride, it.len_in, it.cls) == (2, 4, None)
    it = R.work_item((ST, SP, sig, 1, 7))
    assert (it.sig_stride, it.len_in, it.cls) == (1, 7, "mono")
    it = R.work_item((ST, SP, torch.zeros(6, 2)))
    assert (it.sig_stride, it.len_in, it.cls) == (2, 6, "stereo")
    it = R.work_item((ST, SP, torch.zeros(6, 3)))
    assert (it.sig_stride, it.len_in, it.cls) == (3, 6, None)
    view = torch.zeros(6, 4)[:, :2]
    assert not view.is_contiguous()
    it = R.work_item((ST, SP, view))
    assert (it.sig_stride, it.len_in, it.cls) == (2, 6, None)
    assert R.work_item(it) is it
    assert R.work_item(list((ST, SP, sig))).len_in == 10            # (any sequence, not only tuples)


def test_lookahead_is_pinned():
    assert [R._lookahead(3, g) for g in (1, 4, 8)] == [3, 8, 16]
    assert R._lookahead(8, 8) == 16
    # bench.py's curve ring of 32 relies on "at most 16 items ahead + a group of 8"
    assert max(R._lookahead(P, g) for P in range(1, 9) for g in range(1, 9)) == 16


def test_ring_slots_follow_the_largest_group_of_the_call():
    assert R._GROUP_AUTO == 4
    assert R._ring_slots(3, None) == 16
    assert R._ring_slots(8, None) == 22
    assert R._ring_slots(3, 8) == 32
    assert R._ring_slots(3, 1) == 6
    for P in range(1, 9):
        for group in (None,) + tuple(range(1, 9)):
            # the group sizes the call can choose: `group` or 1 (an item without a class) when given, else what _group_size returns
            for g in ((1, group) if group is not None else (1, R._GROUP_AUTO)):
                assert R._ring_slots(P, group) >= 2 * R._lookahead(P, g), (P, group, g)


def test_group_size_never_exceeds_the_named_constant():
    long_mono = types.SimpleNamespace(cls="mono", n_samples=400_000_000)
    assert R._group_size(mono()) == R._GROUP_AUTO
    assert R._group_size(types.SimpleNamespace(cls="mono", n_samples=399_999_999)) == R._GROUP_AUTO
    assert R._group_size(long_mono) == 1 and R._group_size(stereo()) == 1


def test_int_option(monkeypatch):
    what = "planners / PAR_PLANNERS"
    monkeypatch.delenv("PAR_PLANNERS", raising=False)
    monkeypatch.delenv("PAR_GROUP", raising=False)
    assert R._int_option(None, "PAR_PLANNERS", 3, what) == 3
    assert R._int_option(None, "PAR_GROUP", None, "group / PAR_GROUP") is None
    assert R._int_option(5, "PAR_PLANNERS", 3, what) == 5
    monkeypatch.setenv("PAR_PLANNERS", "2")
    assert R._int_option(None, "PAR_PLANNERS", 3, what) == 2
    assert R._int_option(7, "PAR_PLANNERS", 3, what) == 7           # the argument beats the environment
    for bad, shown in (("x", "'x'"), (0, "0"), (9, "9")):
        with pytest.raises(ValueError) as e:
            R._int_option(bad, "PAR_PLANNERS", 3, what)
        assert str(e.value) == f"planners / PAR_PLANNERS must be an integer 1..8, got {shown}"
    monkeypatch.setenv("PAR_GROUP", "many")
    with pytest.raises(ValueError) as e:
        R._int_option(None, "PAR_GROUP", None, "group / PAR_GROUP")
    assert str(e.value) == "group / PAR_GROUP must be an integer 1..8, got 'many'"
    monkeypatch.setenv("PAR_GROUP", "12")
    with pytest.raises(ValueError) as e:
        R._int_option(None, "PAR_GROUP", None, "group / PAR_GROUP")
    assert str(e.value) == "group / PAR_GROUP must be an integer 1..8, got 12"
    assert R._int_option(1, "PAR_GROUP", None, "group / PAR_GROUP") == 1


def group_sizes(items, group):
    waiting, sizes = list(items), []
    while waiting:
        g, n = R._next_group(waiting, group, True)
        assert 1 <= n <= g
        sizes.append(n)
        del waiting[:n]
    return sizes


def test_grouping_step():
    seq = [mono(), mono(), mono(), stereo(), stereo()] + [mono() for _ in range(5)]
    # groups end at a class change, stereo items go one by one, mono items four at a time
    assert group_sizes(seq, None) == [3, 1, 1, 4, 1]
    assert group_sizes(seq, 2) == [2, 1, 2, 2, 2, 1]                # an override pairs stereo items too
    assert group_sizes(seq, 1) == [1] * 10
    assert group_sizes(seq, 8) == [3, 2, 5]
    long_mono = types.SimpleNamespace(cls="mono", n_samples=400_000_000)
    assert group_sizes([long_mono, long_mono, mono(), mono()], None) == [1, 1, 2]
    strided = R.work_item((ST, SP, torch.zeros(10), 2))
    assert group_sizes([strided, strided, mono()], 8) == [1, 1, 1]  # an item without a class is launched on its own
    # while the iterable may still deliver, a group waits for its items; the head's size comes back for the look-ahead
    assert R._next_group([mono(), mono()], None, False) == (4, 0)
    assert R._next_group([mono(), mono()], None, True) == (4, 2)
    assert R._next_group([mono(), stereo()], None, False) == (4, 0)
    assert R._next_group([mono()] * 4 + [mono()], None, False) == (4, 4)
    assert R._next_group([stereo(), mono()], None, False) == (1, 1)


def test_channel_loop_launches_and_progress(monkeypatch):
    calls, seen = [], []

    def recorder(name):
        def record(*args, **layout):
            # tensors by their offset into the flat view (the channel), everything else as it is
            calls.append((name,) + tuple(a.storage_offset() if torch.is_tensor(a) and a.ndim else a for a in args) + (layout,))
        return record
    for name in ("varispeed_fused_stereo_dev", "varispeed_fused_dev", "sinc_resample_dev", "linear_resample_dev"):
        monkeypatch.setattr(R, name, recorder(name))
    fused, unfused = types.SimpleNamespace(fused_ok=True), types.SimpleNamespace(fused_ok=False)
    pos = torch.tensor(0.0)
    flat_in, flat_out = torch.zeros(40), torch.zeros(30)
    lay = dict(sig_stride=4, len_in=10, out_stride=3)

    def loop(channels, mode, plan, pos_t, progress=True):
        del calls[:], seen[:]
        R.resample_channels(flat_in, flat_out, channels, lay, 32, mode, plan, pos_t, *((seen.append,) if progress else ()))
        return list(calls)

    three = [(0, 0), (3, 1), (1, 2)]
    assert loop(three, "Sinc", fused, None) == [("varispeed_fused_stereo_dev", fused, 0, 3, 32, 0, 1, lay),
                                                  ("varispeed_fused_dev", fused, 1, 32, 2, lay)]
    assert seen == pytest.approx([100 / 3, 200 / 3, 100.0])
    assert loop(three[:2], "Sinc", fused, pos) == [("varispeed_fused_stereo_dev", fused, 0, 3, 32, 0, 1, lay)]    # the plan wins
    assert seen == [50.0, 100.0]
    assert loop(three[:1], "Sinc", fused, None, progress=False) == [("varispeed_fused_dev", fused, 0, 32, 0, lay)] and seen == []
    for plan in (unfused, None):
        assert loop(three, "Sinc", plan, pos) == [("sinc_resample_dev", pos, c_in, 32, c_out, lay) for c_in, c_out in three]
        assert seen == pytest.approx([100 / 3, 200 / 3, 100.0])
    assert loop(three[:2], "Linear", None, pos) == [("linear_resample_dev", pos, c_in, c_out, lay) for c_in, c_out in three[:2]]
    assert seen == [50.0, 100.0]
    assert loop(three[:2], "Cubic", fused, pos) == [] and seen == [50.0, 100.0]     # an unknown mode launches nothing
    assert loop([], "Sinc", fused, None) == [] and seen == []
