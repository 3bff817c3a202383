"""The tap-mode rule of K_sinc's generic loops (csrc/sinc_tap_modes.h) as a table, without the library: tests/sinc_tap_modes_table.cpp
is compiled with the host C++ compiler against that header alone and asked for every NT in 1..512.  What it answers is held against
a float64 restatement of the two error sums written from the mathematics, not from the header: R_n(q) = K/(n^2 - q) on q in [0, 1/4],
K = win_n/pi, against its mid-range constant (error half the range) and against its linear minimax (error half the largest gap
between the chord and the curve, which in closed form is K (1/n - n/g)^2 with g^2 = n^2 (n^2 - 1/4)), each times 2n + 1."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NT_ALL = list(range(1, 513))
BUDGET_LINEAR, BUDGET_CONSTANT = 3e-7, 1.5e-6      # csrc/sinc_block.h, "How R_n(q) ... is evaluated"
CHUNK, FIRST_POLY = 4, 5


def build_table_program(directory):
    exe = os.path.join(str(directory), "sinc_tap_modes_table")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "pyaudiorestoration_amd", "csrc"), os.path.join(ROOT, "tests", "sinc_tap_modes_table.cpp"),
                           "-o", exe])
    return exe


def ask_table(exe, nts):
    out = subprocess.run([exe], input="".join(f"{NT}\n" for NT in nts), capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == 2 * len(nts)
    return {NT: (int(out[2 * i]), int(out[2 * i + 1])) for i, NT in enumerate(nts)}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return ask_table(build_table_program(tmp_path_factory.mktemp("sinc_tap_modes")), NT_ALL)


def pair_errors(NT):
    """(linear, constant): worst-case error of tap pair n = 0..NT-1 in either form (index 0 unused)"""
    n = np.arange(NT, dtype=np.float64)
    K = np.hanning(2 * NT + 1).astype(np.float32)[NT:2 * NT].astype(np.float64) / np.pi
    lin, cst = np.zeros(NT), np.zeros(NT)
    if NT > 1:
        m = n[1:]
        g = np.sqrt(m * m * (m * m - 0.25))
        lin[1:] = 0.5 * K[1:] * (1.0 / m - m / g) ** 2 * (2 * m + 1)
        cst[1:] = 0.5 * K[1:] * 0.25 / (m * m * (m * m - 0.25)) * (2 * m + 1)
    return lin, cst


def test_residues_and_order(table):
    for NT in NT_ALL:
        p1, p0 = table[NT]
        assert p1 % CHUNK == 1 and p0 % CHUNK == 1, (NT, p1, p0)
        assert FIRST_POLY <= p1 <= p0, (NT, p1, p0)


def test_tail_sums_stay_within_the_budgets_and_start_no_later_than_needed(table):
    for NT in NT_ALL:
        p1, p0 = table[NT]
        lin, cst = pair_errors(NT)
        assert lin[p1:].sum() <= BUDGET_LINEAR, (NT, p1, lin[p1:].sum())
        assert cst[p0:].sum() <= BUDGET_CONSTANT, (NT, p0, cst[p0:].sum())
        # one chunk earlier the form would break its budget -- where there is such a chunk: a polynomial one (n0 >= 5) that holds
        # a tap below NT (a form that no chunk uses is reported as starting beyond them all); the constant form cannot start
        # before the linear one
        last = (NT - 1) // CHUNK * CHUNK + 1
        if FIRST_POLY <= p1 - CHUNK <= last:
            assert lin[p1 - CHUNK:].sum() > BUDGET_LINEAR, (NT, p1, lin[p1 - CHUNK:].sum())
        if p1 <= p0 - CHUNK <= last:
            assert cst[p0 - CHUNK:].sum() > BUDGET_CONSTANT, (NT, p0, cst[p0 - CHUNK:].sum())


def test_the_specialised_loops_use_the_same_rule(table):
    """TapTab<32> and TapTab<50> (csrc/sinc_taps_gen.h) are generated with the boundaries the rule gives"""
    assert table[32] == (9, 25) and table[50] == (9, 37)
