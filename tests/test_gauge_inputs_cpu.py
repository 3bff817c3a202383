"""Proofs about tests/gauge_inputs.py, without a GPU: the integer inputs keep every sum exact, every shape reaches the path of
csrc/gauge.hip it is listed for (a replay of the kernel's geometry), the exact FMA-chain emulation differs from
gauge_np.emulate_f32 only where it repairs a double rounding, the exact-variance tolerance sees each index mutation that the old
rounding bound cannot (pytest -s prints the smallest ratio), and par_gauge_frames is the reference's frame count at odd sizes too."""
from fractions import Fraction

import numpy as np
import pytest

import gauge_inputs as I
import gauge_np as G

INT_IDS = [I.shape_id(s) for s in I.ALL_SHAPES]


# ------------------------------------------------------------------------------------------------------------ input proofs

@pytest.mark.parametrize("shape", I.ALL_SHAPES, ids=INT_IDS)
def test_integer_inputs_keep_every_sum_exact(shape):
    n_fft, hop, n = shape
    c = I.int_case(shape)
    for a, cap in ((c.x, 4), (c.h_re, 8), (c.h_im, 8)):
        assert a.dtype == np.float32 and np.array_equal(a, np.rint(a)) and np.max(np.abs(a)) <= cap
    assert np.any(c.x != 0) and np.any(c.h_re != 0) and np.any(c.h_im != 0)
    assert n_fft * 4 * 8 < 2 ** 24                                   # every partial sum of a tap chain, in any order
    worst = 1.0
    for i, ((zr, zi), m) in enumerate(zip(c.z, c.moments)):
        sr, si, s2, F = m
        assert F == I.frames(n, n_fft, hop, i) == len(zr)
        assert int(np.abs(zr).sum()) < 2 ** 53 and int(np.abs(zi).sum()) < 2 ** 53 and s2 < 2 ** 53
        var = I.variance(m)
        if F == 1:                                                   # one frame: the variance is 0 whatever the frame holds
            assert var == 0
            continue
        # var >= S2 / (2 F): the tolerance is 16 * 2^-53 = 1.8e-15 of the variance at most, a large mean cannot inflate it
        assert var >= Fraction(s2, 2 * F), (shape, i, float(var), s2 / F)
        if s2:
            worst = min(worst, float(var / Fraction(s2, F)))
    print(f"\n{shape}: smallest var / (S2 / F) over the pads {worst:.3f}")


def test_delta_inputs_tell_the_ends_apart():
    for shape in I.shapes_of(*I.DELTA_GROUPS) + [G.IMPULSE_SHAPE]:
        n_fft, hop, n = shape
        x, mom = I.delta_moments(shape)
        ends = [x[0], x[1], x[n - 2], x[n - 1]]
        assert len(set(ends)) == 4 and all(abs(v) in (3.0, 4.0) for v in ends) and np.max(np.abs(x)) <= 4
        ms = I.delta_taps(n_fft)
        want = {0, 7, 8, 15, 16, n_fft - 2, n_fft - 1} | ({1023, 1024, 1039, 1040} if n_fft > 1024 else set())
        assert set(ms) == {m for m in want if 0 <= m < n_fft} and {0, n_fft - 1} <= set(ms)
        assert set(mom) == {(m, part) for m in ms for part in (0, 1)}
        for (m, part), per_pad in mom.items():
            hr, hi = I.delta_filter(n_fft, m, part)
            assert hr.sum() + hi.sum() == 1.0 and (hr, hi)[part][m] == 1.0
            i = (m * 7 + part) % hop                                 # one pad per filter against the matrix product
            assert per_pad[i] == I.moments(*I.exact_z(x, hr, hi, n_fft, hop, i))


# --------------------------------------------------------------------------------------------------------- geometry replay

def _reaches(shape):
    """what the replay must show for the shape's group"""
    n_fft, hop, n = shape
    g = I.Geometry(*shape)
    group = next(k for k, v in I.SHAPES.items() if shape in v)
    rotates = any(g.rotation(w) != 0 for w in range(1, g.n_wg))
    skipped = any(g.slot(i, w) >= g.slots for i in range(hop) for w in range(g.n_wg))
    runs = g.lane_runs()
    if group == "rotation":
        return g.n_wg == 3 and rotates and I.TILE % hop != 0 and n_fft % I.TAP_BLOCK == 2 and len(g.chunks) == 1
    if group == "slots_stride":
        return I.BLOCK < hop < I.TILE and g.n_wg == 3 and rotates and g.slots == hop
    if group == "hop_over_tile":
        return hop > I.TILE and g.slots == I.TILE and skipped and g.n_wg in (4, 5) and rotates
    if group == "final_runs":
        cut = any(lo < g.n_wg < lo + g.per for lo, hi in runs)
        empty = any(lo >= hi for lo, hi in runs)
        return g.per == 2 and empty and g.n_wg == {526341: 257, 614400: 300}[n] and cut == (g.n_wg == 257)
    if group == "chunk_tail":
        return g.chunks == {1030: [1024, 6], 2050: [1024, 1024, 2]}[n_fft] and g.chunks[-1] < I.TAP_BLOCK
    if group == "no_dense":
        return g.dense == 0 and g.n_wg == 0 and all(g.j_lo(i) > g.j_hi(i) for i in range(hop))
    if group == "tile_seam":
        return g.dense == n and g.n_wg == (2 if n > I.TILE else 1)
    if group == "odd":
        return n_fft % 2 == 1 and any((n + i + n_fft // 2) % hop == 0 for i in range(hop)) and (hop < I.TILE or g.slots == I.TILE)
    return True


@pytest.mark.parametrize("shape", I.ALL_SHAPES, ids=INT_IDS)
def test_replay_shape_reaches_its_path_and_covers_every_frame_once(shape):
    n_fft, hop, n = shape
    g = I.Geometry(*shape)
    assert _reaches(shape), shape
    assert (shape in I.MULTI_WG_SHAPES) == (g.n_wg > 1)
    pads = range(hop) if hop <= 64 else sorted({0, 1, 2, hop // 2, hop - 2, hop - 1} | set(range(0, hop, max(1, hop // 37))))
    for i in pads:
        assert g.covers_every_frame_once(i), (shape, i)
        assert g.covers_by_count(i)
        dense_j, edge_j = g.frame_sources(i)
        assert len(dense_j) == max(0, g.j_hi(i) - g.j_lo(i) + 1) and len(edge_j) <= g.edges
        assert np.all(g.workgroup_of(i, dense_j) >= 0) and np.all(g.workgroup_of(i, edge_j) == -1)
    if n_fft % 2 and hop < I.TILE:                                   # the pads where the old count ran one frame too far
        hit = [i for i in range(hop) if (n + i + n_fft // 2) % hop == 0]
        assert hit and all((n + i + n_fft // 2) // hop + 1 == g.frames(i) + 1 for i in hit)


def test_replay_edge_lanes_suffice_at_every_small_shape():
    """ga_geometry's edge count against the frame count, odd and even n_fft: every pad of 27,456 shapes"""
    shapes = pads = 0
    for n_fft in range(2, 26):
        for hop in range(1, 27):
            for n in list(range(1, 41)) + [53, 64, 97, 128]:
                g = I.Geometry(n_fft, hop, n)
                shapes += 1
                for i in range(hop):
                    pads += 1
                    assert g.covers_by_count(i), (n_fft, hop, n, i)
    for shape in [(3, 5000, 4097), (5, 2049, 4100), (4097, 4097, 9000), (7, 2047, 6143), (2049, 3, 2060)]:   # across the tile
        g = I.Geometry(*shape)
        for i in range(0, shape[1], 7):
            assert g.covers_every_frame_once(i), (shape, i)
    print(f"\n{shapes} shapes, {pads} pads")


# ----------------------------------------------------------------------------------------------------- the exact FMA chain

def test_tie_repair_on_a_constructed_double_rounding():
    """acc = 2^30 + 128 (float32 spacing 128, odd significand) plus (8 + 2^-20)(8 - 2^-20) = 64 - 2^-40: float64 rounds the sum ONTO
    the float32 midpoint 2^30 + 192 and rounding that to float32 goes to the even 2^30 + 256; the FMA's single rounding sees a value
    below the midpoint and gives 2^30 + 128."""
    acc = 2.0 ** 30 + 128.0
    P = np.array([[acc], [8.0 + 2.0 ** -20]])
    h = np.array([1.0, 8.0 - 2.0 ** -20])
    assert np.array_equal(P.astype(np.float32), P) and np.array_equal(h.astype(np.float32), h)
    for sign in (1.0, -1.0):
        got, k, _ = I.fma_chain(sign * P, h)
        naive, k0, _ = I.fma_chain(sign * P, h, repair=False)
        assert float(got[0]) == sign * acc and k == 1
        assert float(naive[0]) == sign * (acc + 128.0) and k0 == 0
    # a true tie (product exactly 64) goes to even in both
    P[1, 0], h[1] = 8.0, 8.0
    for repair in (True, False):
        got, k, _ = I.fma_chain(P, h, repair=repair)
        assert float(got[0]) == acc + 128.0 and k == 0


@pytest.mark.parametrize("name", I.REAL_SHAPES)
def test_exact_chain_equals_the_rounded_emulation_but_for_its_repairs(name):
    n_fft, hop, n = G.GPU_SHAPES[name]
    x, hr, hi, z, repaired, smallest = I.real_case(name)
    z0, none, _ = I.emulate_chain(x, hr, hi, n_fft, hop, repair=False)
    assert none == 0
    assert smallest >= 2.0 ** -126                                   # no partial sum is subnormal: the denormal mode cannot matter
    old = G.emulate_f32(x, hr, hi, n_fft, hop)
    assert np.array_equal(np.array([I.std_naive(*p) for p in z0]), old)        # the unrepaired chain IS gauge_np.emulate_f32
    differ = sum(int(np.count_nonzero((a != c) | (b != d))) for (a, b), (c, d) in zip(z, z0))
    print(f"\n{name}: {repaired} of {2 * n_fft * sum(len(a) for a, _ in z)} steps repaired, {differ} z differ, "
          f"smallest partial sum {smallest:.3e}")
    assert differ <= repaired


# -------------------------------------------------------------------------------------------------------------------- power

def _mutants(c, g):
    """name -> [(pad, mutated moments)]: the index errors the old tolerance cannot see, applied to the exact oracle"""
    n_fft, hop, n = c.shape
    out = {k: [] for k in ("drop_first", "drop_last", "duplicate_dense", "F_plus_1", "next_class", "no_right_reflection",
                           "no_left_reflection", "class_shift_after_wg0")}

    def mom(zr, zi, F):
        return I.moments(zr, zi)[:3] + (F,)

    dense = []                                                       # per pad: (sum re, sum im, sum |z|^2) of the dense frames
    later = []                                                       # ... and of those in workgroups 1, 2, ..
    for i in range(hop):
        zr, zi = c.z[i]
        w = g.workgroup_of(i, np.arange(len(zr)))
        dense.append(I.moments(zr[w >= 0], zi[w >= 0])[:3])
        later.append(I.moments(zr[w >= 1], zi[w >= 1])[:3])
    for i in range(hop):
        zr, zi = c.z[i]
        sr, si, s2, F = c.moments[i]
        out["drop_first"].append((i, mom(zr[1:], zi[1:], F)))
        out["drop_last"].append((i, mom(zr[:-1], zi[:-1], F)))
        if g.j_lo(i) <= g.j_hi(i):
            k = (g.j_lo(i) + g.j_hi(i)) // 2
            out["duplicate_dense"].append((i, mom(np.append(zr, zr[k]), np.append(zi, zi[k]), F)))
        out["F_plus_1"].append((i, (sr, si, s2, F + 1)))
        for name, part in (("next_class", dense), ("class_shift_after_wg0", later)):
            a, b = part[i], part[(i + 1) % hop]
            out[name].append((i, (sr - a[0] + b[0], si - a[1] + b[1], s2 - a[2] + b[2], F)))
        for name, blank, js in (("no_left_reflection", dict(zero_left=True), [j for j in range(F) if j * hop < g.half]),
                                ("no_right_reflection", dict(zero_right=True),
                                 [j for j in range(max(0, F - g.half // hop - 2), F) if j * hop + n_fft > n + i + 2 * g.half])):
            if js:
                ar, ai = zr.copy(), zi.copy()
                ar[js], ai[js] = I.exact_z(c.x, c.h_re, c.h_im, n_fft, hop, i, js=js, **blank)
                out[name].append((i, mom(ar, ai, F)))
    return out


@pytest.mark.parametrize("shape", I.ALL_SHAPES, ids=INT_IDS)
def test_tolerance_sees_every_index_mutation(shape):
    """A mutation touches a pad when it changes what the statistic is a function of, that pad's exact (|S|^2, S2, F) -- dropping a
    frame of structural zeros or swapping classes where there is no dense frame is the same computation, and std does not see the
    phase of z: on a pad of one zero and one non-zero frame a swap that keeps |z| keeps the variance --, the pad has more than one
    frame (the variance of a single frame is 0 whatever it holds; only F + 1 moves it) and its series is not all zeros before and
    after (then every statistic is 0 for any F).  On every pad it touches, the variance must move by more than 1000 tolerances."""
    c, g = I.int_case(shape), I.Geometry(*shape)
    smallest, report = np.inf, []
    for name, pads in _mutants(c, g).items():
        if name == "class_shift_after_wg0" and shape not in I.MULTI_WG_SHAPES:
            continue
        touched = 0
        for i, m in pads:
            o = c.moments[i]
            same = (m[0] ** 2 + m[1] ** 2, m[2], m[3]) == (o[0] ** 2 + o[1] ** 2, o[2], o[3])
            if same or (m[3] == 1 and o[3] == 1) or (m[2] == 0 and o[2] == 0):
                continue
            touched += 1
            moved, tol = abs(I.variance(m) - I.variance(c.moments[i])), I.tolerance(c.moments[i])
            ratio = float(moved / tol) if tol else (np.inf if moved else 0.0)      # an all-zero pad: the tolerance is 0
            assert ratio > 1000.0, (shape, name, i, ratio)
            smallest = min(smallest, ratio)
        report.append(f"{name} {touched}/{len(pads)}")
        # with frames that overlap by half or more and a dense part, every mutation is seen on some pad
        assert touched > 0 or shape[1] > shape[0] // 2 or g.dense == 0, (shape, name)
        if name in ("next_class", "class_shift_after_wg0", "duplicate_dense", "F_plus_1") and g.dense > 0:
            assert touched > 0, (shape, name, touched)
    print(f"\n{shape}: smallest move / tolerance {smallest:.3g}; pads touched: " + ", ".join(report))


# -------------------------------------------------------------------------------------------------------------- frame count

FRAME_SHAPES = [(203, 51, 4), (5000, 51, 7), (5, 3, 2), (4097, 3, 5000), (40, 2050, 5), (333, 50, 7), (1000, 64, 8), (199, 51, 4),
                (1, 3, 1), (7, 5, 3)]


@pytest.mark.parametrize("n,n_fft,hop", FRAME_SHAPES)
def test_gauge_frames_is_the_reference_count_at_odd_and_even_sizes(n, n_fft, hop):
    from pyaudiorestoration_amd import _lib
    L = _lib.lib()
    pads = {0, 1 % hop, hop // 2, hop - 1}
    pads |= {i for i in range(hop) if (n + i + n_fft // 2) % hop == 0 and (i < 8 or hop - i < 8)}   # hop | M: where odd sizes differed
    assert any((n + i + n_fft // 2) % hop == 0 for i in pads) or hop > n + n_fft
    for off in sorted(pads):
        want = len(G.frames_of(G.padded(np.zeros(n), off, n_fft), n_fft, hop))
        assert I.frames(n, n_fft, hop, off) == want
        assert L.par_gauge_frames(n, n_fft, hop, off) == want, (n, n_fft, hop, off)
