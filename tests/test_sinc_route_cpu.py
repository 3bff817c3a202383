"""The routing rule of K_sinc (csrc/sinc_route.h) as a table, without the library: tests/sinc_route_table.cpp is compiled with the
host C++ compiler against that header alone, fed rows of integers (pointers as integers, so alignment and sig1 == sig0 + 1 can
be set freely) and its answers are compared with the routes written out here by hand, from include/par_hip.h's "Which kernel
runs" -- nothing below recomputes the rule."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIG, OUT = 4096, 8192            # addresses; the next float lies 4 bytes on


def item(len_out=4096, len_in=4096, sig0=SIG, sig1=0, sig_stride=1, out0=OUT, out1=0, out_stride=1):
    return (len_out, len_in, sig0, sig1, sig_stride, out0, out1, out_stride)


def stereo(**kw):
    return item(**dict(dict(sig1=SIG + 4, sig_stride=2, out1=OUT + 4, out_stride=2), **kw))


# (item, NT, streaming allowed) -> route
SINGLE = [
    (item(), 32, 1, "StreamMono"),
    (item(len_out=4095), 32, 1, "Block"),
    (item(len_in=4095), 32, 1, "Block"),
    (item(len_out=4095, len_in=4095), 32, 1, "Block"),
    (item(len_out=4096, len_in=4096), 32, 1, "StreamMono"),
    (item(len_out=1 << 33, len_in=1 << 33), 32, 1, "StreamMono"),
    (item(), 50, 1, "Block"),
    (item(), 16, 1, "Block"),
    (item(), 32, 0, "Block"),
    (item(sig_stride=1, out_stride=1), 32, 1, "StreamMono"),
    (item(sig_stride=2, out_stride=1), 32, 1, "StreamPick"),
    (item(sig_stride=2, out_stride=2), 32, 1, "StreamPick"),
    (item(sig_stride=2, out_stride=3), 32, 1, "StreamPick"),
    (item(sig_stride=3, out_stride=1), 32, 1, "Block"),
    (item(sig_stride=1, out_stride=2), 32, 1, "Block"),
    (item(sig_stride=2, out_stride=2, len_out=4095), 32, 1, "Block"),
    (item(sig_stride=2, out_stride=2), 50, 1, "Block"),
    (item(sig_stride=2, out_stride=2), 32, 0, "Block"),
    (stereo(), 32, 1, "StreamStereo"),
    (stereo(out0=OUT + 8, out1=OUT + 12), 32, 1, "StreamStereo"),
    (stereo(out0=OUT + 4, out1=OUT + 8), 32, 1, "Block"),                 # out0 at 4 mod 8
    (stereo(sig0=SIG + 4, sig1=SIG + 8), 32, 1, "StreamStereo"),          # (the input may sit anywhere)
    (stereo(sig1=SIG + 40000), 32, 1, "Block"),                           # planar sig1
    (stereo(out1=OUT + 40000), 32, 1, "Block"),                           # planar out1
    (stereo(sig1=SIG - 4), 32, 1, "Block"),                               # the channels the other way round
    (stereo(out_stride=1), 32, 1, "Block"),                               # sig_stride 2 with out_stride 1
    (stereo(sig_stride=1), 32, 1, "Block"),
    (stereo(sig_stride=3, out_stride=3), 32, 1, "Block"),
    (stereo(len_out=4095), 32, 1, "Block"),
    (stereo(len_in=4095), 32, 1, "Block"),
    (stereo(), 50, 1, "Block"),
    (stereo(), 16, 1, "Block"),
    (stereo(), 32, 0, "Block"),
    # exactly one of sig1 / out1: one channel, the lone pointer is not looked at
    (item(sig1=SIG + 4), 32, 1, "StreamMono"),
    (item(out1=OUT + 4), 32, 1, "StreamMono"),
    (item(sig1=SIG + 4, sig_stride=2, out_stride=2), 32, 1, "StreamPick"),
    (item(out1=OUT + 4, sig_stride=2, out_stride=2), 32, 1, "StreamPick"),
    (item(sig1=SIG + 4, sig_stride=3), 32, 1, "Block"),
]

# (items, NT, streaming allowed) -> StreamMono / StreamStereo: merge the launches; Block: item by item
BATCH = [
    ([item()], 32, 1, "Block"),                                                           # n = 1
    ([stereo()], 32, 1, "Block"),
    ([item(), item(len_out=5000, len_in=7000), item(len_out=1 << 20, len_in=1 << 20)], 32, 1, "StreamMono"),
    ([stereo(), stereo(len_out=9999, len_in=9000)], 32, 1, "StreamStereo"),
    ([item(), stereo()], 32, 1, "Block"),
    ([stereo(), item()], 32, 1, "Block"),
    ([item(), item(len_out=4095), item()], 32, 1, "Block"),                               # one item below the threshold
    ([item(len_in=4095), item()], 32, 1, "Block"),
    ([stereo(), stereo(len_out=4095)], 32, 1, "Block"),
    ([item(), item(sig_stride=2), item()], 32, 1, "Block"),                               # one StreamPick item
    ([item(sig_stride=2), item(sig_stride=2)], 32, 1, "Block"),                           # StreamPick never merges
    ([stereo(), stereo(out0=OUT + 4, out1=OUT + 8)], 32, 1, "Block"),                     # one misaligned stereo item
    ([stereo(out0=OUT + 4, out1=OUT + 8), stereo()], 32, 1, "Block"),
    ([item(), item()], 50, 1, "Block"),
    ([stereo(), stereo()], 50, 1, "Block"),
    ([item(), item()], 32, 0, "Block"),                                                   # streaming not allowed
    ([stereo(), stereo()], 32, 0, "Block"),
    ([item(len_out=4096 + 100 * k, len_in=5000 + k) for k in range(9)], 32, 1, "StreamMono"),     # n = 9
    ([stereo()] * 9, 32, 1, "StreamStereo"),
    ([item()] * 8 + [stereo()], 32, 1, "Block"),
    ([item()] * 8 + [item(sig_stride=3)], 32, 1, "Block"),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sinc_route") / "sinc_route_table")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "pyaudiorestoration_amd", "csrc"), os.path.join(ROOT, "tests", "sinc_route_table.cpp"),
                           "-o", exe])

    def ask(kind, rows):
        text = "".join(f"{kind} {NT} {allowed} {len(items)} " + " ".join(str(v) for it in items for v in it) + "\n"
                       for items, NT, allowed, _ in rows)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == len(rows)
        return out
    return ask


def test_single_rule(driver):
    rows = [([it], NT, allowed, want) for it, NT, allowed, want in SINGLE]
    for row, got in zip(rows, driver("S", rows)):
        assert got == row[3], row


def test_batch_rule(driver):
    for row, got in zip(BATCH, driver("B", BATCH)):
        assert got == row[3], row
    # the batch rule of a lone streamable item is "item by item", whatever the single rule says of it
    assert driver("S", [([item()], 32, 1, None)]) == ["StreamMono"]
