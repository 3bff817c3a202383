"""Scalar bookkeeping of the streaming kernel's hot loops, from the compiler's gfx950 listing (no GPU): how many scalar
instructions one iteration issues -- the `salu` column of tools/isa_census.py, which counts by instruction class and looks for
no particular instruction -- and the registers, scratch and occupancy the two mono kernels are built around.

Bounds.  Before r09 an iteration of k_sinc_pipe<1, 2> issued 172 / 164 / 165 scalar instructions (order 6 / fc = 1 / order 5) and
k_sinc_pipe<1, 1> 159.  The caps of the r09 issue hold whatever the build reaches: at most 135 in every hot loop of <1, 2>, at most
130 in <1, 1>.  The pins are what r09 reached (129 / 119 / 122 and 112, profiles/r09_isa_census.txt) plus 4.  Registers: <1, 2>
at most 216 (two waves per SIMD leave 256; the loop order of r08 is built on 211), <1, 1> at most 128 (four waves per SIMD); no
scratch."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAP = {"2": 135, "1": 130}
REACHED = {"2": {"order6": 129, "unity": 119, "order5": 122}, "1": {"unity": 112}}


@pytest.fixture(scope="module")
def census():
    spec = importlib.util.spec_from_file_location("isa_census", os.path.join(ROOT, "tools", "isa_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    L, files, stages = mod.compile_listing([])
    return mod, L, files, stages


def _loops(census, kind):
    """{loop name: {class: instructions per iteration}} of k_sinc_pipe<1, kind>; the loops are told apart by their MFMAs"""
    mod, L, files, stages = census
    _, loops = mod.kernel_loops(L, "1", kind)
    out = {}
    for h, back in loops:
        tot = mod.loop_totals(mod.loop_census(L, h, back, files, stages))
        name = "unity" if tot["mfma"] <= 16 else ("order5" if tot["mfma"] <= 29 else "order6")
        assert name not in out, (name, tot)
        out[name] = tot
    return out


@pytest.mark.parametrize("kind", ["2", "1"])
def test_scalar_instructions_per_iteration(census, kind):
    loops = _loops(census, kind)
    assert sorted(loops) == sorted(REACHED[kind]), sorted(loops)
    for name, tot in loops.items():
        print(f"k_sinc_pipe<1, {kind}> {name}: {tot['salu']} scalar instructions per iteration")
    for name, tot in loops.items():
        assert tot["salu"] <= CAP[kind], (name, tot)
        assert tot["salu"] <= REACHED[kind][name] + 4, (name, tot)


def test_registers_scratch_occupancy(census):
    mod, L, _, _ = census
    two, _ = mod.kernel_loops(L, "1", "2")
    assert two["NumVgprs"][0] <= 216 and two["ScratchSize"][0] == 0 and two["Occupancy"][0] == 2, two
    four, _ = mod.kernel_loops(L, "1", "1")
    assert four["NumVgprs"][0] <= 128 and four["ScratchSize"][0] == 0 and four["Occupancy"][0] == 4, four
