"""Static checks of the streaming kernel's mono hot loops, from the compiler's gfx950 listing (no GPU): the registers and
occupancy the two kernel kinds are built around and one memory wait per iteration -- for the default build and for
-DPAR_S3_EARLY_LDS=1 -- and, for the latter, the order of an iteration of k_sinc_pipe<1, 2>: every LDS read issued a stage
ahead of its use (csrc/sinc2.hip, "Order of one iteration").

Bounds.  An LDS read comes back after ~64 (ds_read_b32) to ~128 cycles (a wave's six ds_read_b128 behind one another); the
parent order put 0-4 of the wave's own vector instructions (<= 16 priced port cycles) between a read of the records, the ring
chunk or the image fragments and the wait for it.  Asked for here: at least 128 priced port cycles of the wave's own vector
work behind the chunk's and every fragment read, and at least 8 vector instructions (twice the parent's best case) behind the
records -- PLACE needs them first, only the other reads' address arithmetic can stand between."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_LISTINGS = {}


def _listing(build):
    if build not in _LISTINGS:
        _LISTINGS[build] = _compile(build)
    return _LISTINGS[build]


@pytest.fixture(scope="module", params=["default", "early"])
def census(request):
    return _listing(request.param)


@pytest.fixture(scope="module")
def census_early():
    return _listing("early")


def _compile(build):
    spec = importlib.util.spec_from_file_location("isa_census", os.path.join(ROOT, "tools", "isa_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    L, files, stages = mod.compile_listing(["-DPAR_S3_EARLY_LDS=1"] if build == "early" else [])
    return mod, L, files, stages


def test_registers_and_occupancy(census):
    mod, L, _, _ = census
    two, _ = mod.kernel_loops(L, "1", "2")
    assert two["Occupancy"][0] == 2 and two["NumVgprs"][0] <= 256 and two["ScratchSize"][0] == 0, two
    four, _ = mod.kernel_loops(L, "1", "1")
    assert four["Occupancy"][0] == 4 and four["ScratchSize"][0] == 0, four


@pytest.mark.parametrize("kind", ["2", "1"])
def test_one_memory_wait_per_iteration(census, kind):
    mod, L, _, _ = census
    _, loops = mod.kernel_loops(L, "1", kind)
    assert len(loops) == (3 if kind == "2" else 1)          # fc < 1 to order 6, fc = 1, fc < 1 to order 5 / fc = 1
    for h, back in loops:
        assert sum(1 for i in range(h, back + 1) if re.search(r"s_waitcnt.*vmcnt", L[i])) == 1


def test_lds_reads_a_stage_ahead(census_early):
    mod, L, files, stages = census_early
    _, loops = mod.kernel_loops(L, "1", "2")
    for h, back in loops:
        rows = mod.waits_rows(L, h, back, files, stages)
        by_stage = {}
        for ln, txt, st, wl, n, nv, pc in rows:
            by_stage.setdefault(st, []).append((txt, nv, pc))
        # (how many reads the compiler makes of them is its business: every one found is held to the bound)
        assert by_stage.get("place") and by_stage.get("convert") and by_stage.get("bank"), by_stage
        for txt, nv, pc in by_stage["place"]:
            assert nv >= 8, (txt, nv, pc)
        for txt, nv, pc in by_stage["convert"] + by_stage["bank"]:
            assert pc >= 128.0, (txt, nv, pc)
