"""Vector-port bookkeeping of the streaming kernel's hot loops, from the compiler's gfx950 listing (no GPU): how many vector ALU
instructions one iteration issues -- the `valu` column of tools/isa_census.py, which counts by instruction class and looks for
no particular instruction -- and what the listing model prices them at (printed, not asserted: the prices are a model).

Bounds.  Before r10 an iteration of k_sinc_pipe<1, 2> issued 353 / 249 / 345 vector instructions (order 6 / fc = 1 / order 5) and
k_sinc_pipe<1, 1> 253 (profiles/r09_isa_census.txt).  The caps of the r10 issue hold whatever the build reaches: every loop of
<1, 2> at least 6 below its parent, <1, 1> at least 8 below -- what the stores off a scalar base, the carried `c - ws`, the rows'
flags in one test, `t5` handed over and the conversion verdict's ballots remove statically (the branch of the tile anchor's
scalar case counts against them).  The pins are what r10 reached (316 / 214 / 308 and 217, profiles/r10_isa_census.txt) plus 2.
The counted range is the loop from its header to its back edge; the block of the pass that straddles a tile border (8 vector and
3 scalar instructions, one pass in eight) is laid out of line behind it and not counted -- with it every figure still clears
its cap."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARENT = {"2": {"order6": 353, "unity": 249, "order5": 345}, "1": {"unity": 253}}
BELOW = {"2": 6, "1": 8}
REACHED = {"2": {"order6": 316, "unity": 214, "order5": 308}, "1": {"unity": 217}}


@pytest.fixture(scope="module")
def census():
    spec = importlib.util.spec_from_file_location("isa_census", os.path.join(ROOT, "tools", "isa_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    L, files, stages = mod.compile_listing([])
    return mod, L, files, stages


def _loops(census, kind):
    """{loop name: {class: instructions per iteration, "port": priced port cycles}} of k_sinc_pipe<1, kind>; the loops are told
    apart by their MFMAs"""
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
def test_vector_instructions_per_iteration(census, kind):
    loops = _loops(census, kind)
    assert sorted(loops) == sorted(REACHED[kind]), sorted(loops)
    for name, tot in loops.items():
        print(f"k_sinc_pipe<1, {kind}> {name}: {tot['valu']} vector instructions per iteration (parent {PARENT[kind][name]}), "
              f"{tot['port']:.0f} priced port cycles")
    for name, tot in loops.items():
        assert tot["valu"] <= PARENT[kind][name] - BELOW[kind], (name, tot)
        assert tot["valu"] <= REACHED[kind][name] + 2, (name, tot)
