"""Preconditions of tests/plan_ladder_inputs.py, without a GPU: for every case the reference accepts or refuses the curve as the table
says, predict() yields the case's literal ladder, and the curve has what its rung hangs on -- the near-ties (how many, exactly ON the
tie, every other sum far from the zone), the product outside the range, the segments a lazy plan refuses, the long segments, the count
of offsets at or below zero, the buffer bound on or far from an integer, the two equidistant positions of the trim -- and stays clear
of the rungs it is not about.  A disagreement on the GPU is then the library's."""
import functools

import numpy as np
import pytest

import plan_ladder_inputs as P

NAMES = list(P.CASES)
ZONE = float(P.TIE_ZONE)


@functools.lru_cache(maxsize=None)
def _predicted(name):
    return P.CASES[name].predict()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(positions, trimmed) of the numpy oracle, or the exception it raises"""
    from oracle import oracle_np as O
    c = P.CASES[name]
    try:
        with np.errstate(all="ignore"):
            return O.speed_to_pos(c.st, c.sp, c.n_in)
    except (IndexError, ValueError, ZeroDivisionError) as e:
        return e


@pytest.mark.parametrize("name", NAMES)
def test_reference_accepts_or_raises_as_the_table_says(name):
    from oracle import oracle_c as C
    c, ref = P.CASES[name], _reference(name)
    if c.raises:
        assert isinstance(ref, IndexError), ref                       # seg[-1] of an empty segment (util/resampling.py:126)
        with pytest.raises(ValueError):
            C.speed_to_pos(c.st, c.sp, c.n_in)
        return
    pos, trimmed = ref
    want_c, trimmed_c = C.speed_to_pos(c.st, c.sp, c.n_in)            # what the GPU test compares with: the same bits
    assert trimmed == trimmed_c and np.array_equal(pos.view(np.int64), want_c.view(np.int64))
    r = _predicted(name)
    assert len(pos) == r["len_out"] and trimmed == r["trimmed"], (len(pos), r["len_out"])
    assert c.len_out is None or len(pos) == c.len_out, (len(pos), c.len_out)
    assert len(pos) <= 2_100_000                                       # the GPU test stays quick


@pytest.mark.parametrize("name", NAMES)
def test_predict_yields_the_ladder_of_the_table(name):
    c, r = P.CASES[name], _predicted(name)
    assert r["goes"] == c.goes, r["goes"]
    assert r["raises"] == c.raises
    if not c.raises:
        assert (r["path"], r["flags"], r["fused_ok"], r["n_long"]) == (c.path, c.flags, c.fused_ok, c.n_long), r
        assert r["lazy"] == (c.fused_ok == 2)
    if c.plain is not None:
        q = c.predict_plain()
        assert (q["goes"], q.get("path"), q.get("flags")) == tuple(c.plain), q
    m = len(c.sp)
    assert (c.goes[0].startswith("lazy")) == (not c.kwargs.get("eager") and not c.kwargs.get("force_host_chain")
                                               and c.n_in // (m - 1) <= P.K_LAZY_MAX_N)


@pytest.mark.parametrize("name", NAMES)
def test_each_case_has_its_rung_and_is_clear_of_the_others(name):
    c, r = P.CASES[name], _predicted(name)
    # near-ties: exactly on k + 1/2 where the case is about them (the library's zone is 2^-32 wide), and no cumulative length of any case
    # within 1000 zones of its edge otherwise
    want_ties = {"lazy-length-ties": 1500, "lazy-length-ties-odd": 1500, "eager-length-ties": 1500, "mixed-long-length-ties": 33, "sparse-length-tie": 1,
                 "cap-ambiguous-and-ties": 1000}
    assert r["ties"] == want_ties.get(name, 0) and (name in P.TIE_CASES) == (r["ties"] > 0)
    assert r["tie_margin"] > 1000 * ZONE, r["tie_margin"]
    a = P.products(c.st, c.sp)
    if r["ties"]:
        run = np.cumsum(a)                                            # (exact here: multiples of 1/2 below 2^53)
        assert int(np.sum(run - np.floor(run) == 0.5)) == r["ties"]
        # the scan sends a sum on the tie down, Python's round() the recurrence's to even: other lengths where a period's floor is odd
        assert r["lengths_agree"] == (name != "lazy-length-ties-odd")
    else:
        assert r["lengths_agree"]                                     # and the device's lengths are the reference's
    # the product outside [2^-11, 2^62)
    assert r["in_range"] == (name not in P.RANGE_CASES)
    if name in P.RANGE_CASES:
        bad = np.nonzero(~((a >= P.A_MIN) & (a < P.A_MAX)))[0]
        assert list(bad) == [49 if name == "range-in-front" else 149] and 0.0 <= a[bad[0]] < P.A_MIN
        assert "serial" in c.goes and r.get("bad_segment", None) == (49 if c.raises else None)
        if not c.raises:
            assert r["first_bad"] == 149 and r["trim_seg"] is not None and r["trim_seg"] < 149       # behind the trim
    # the buffer bound: on the integer, or at least 1000 of the test's thresholds away from one
    if name in P.CAP_CASES:
        assert r["cap_dist"] <= r["cap_thr"] / 2 and (c.raises or c.kwargs.get("force_host_chain") or c.flags & P.FLAG_CAP_AMBIGUOUS)
    else:
        assert r["cap_dist"] >= 1000 * r["cap_thr"] and not (c.flags or 0) & P.FLAG_CAP_AMBIGUOUS
    # offsets at or below zero, and binade crossings: beyond the stitch's table by hundreds, or inside it by hundreds
    if not c.kwargs.get("force_host_chain"):
        direct = r["nonpos"] + r["crossing"]
        if name == "direct-overflow":
            assert r["nonpos"] == 2344 and direct >= P.K_MAX_DIRECT + 256
        elif name == "direct-many":
            assert r["nonpos"] == 1563 and direct <= P.K_MAX_DIRECT - 256
        else:
            assert direct <= 64, direct
    # long segments, and the segments a lazy plan refuses
    if c.goes != ["serial"]:
        assert (r["n_long_segments"] > 0) == any("+long" in g for g in c.goes)
        if c.goes[0].startswith("lazy"):
            assert r["lazy_segments_ok"] == (not any(g.startswith("eager") for g in c.goes))
    # the trim: two positions equally far from n_in (equal as float64), one position on it, or neither
    if name in P.TRIM_TIE_CASES or name == "serial-with-long-trim-sparse":
        assert r["trim_min"] == (0.25, 2) and r["trimmed"]
    elif name == "trim-exact-hit":
        assert r["trim_min"] == (0.0, 1)
    elif name == "no-trim":
        assert r["trim_min"] is None and not r["trimmed"]
    elif not c.raises:
        assert r["trimmed"] and r["trim_min"][1] == 1
    # the checkpoint buffer: too small only where the case says so
    if not c.raises:
        assert (r["len_out"] > r["max_out"]) == name.startswith("ck-overflow")
        if name.startswith("ck-overflow"):
            assert r["max_out"] == r["len_out"] // 2


def test_header_words_and_constants_match_the_sources():
    """the constants restated by value are the ones the sources hold, and the header words are where PlanHeader puts them"""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyaudiorestoration_amd", "csrc")
    src = open(os.path.join(root, "pos_plan.h")).read() + open(os.path.join(root, "pos.hip")).read() + \
        open(os.path.join(root, "par_common.h")).read()

    def const(name):
        return re.search(r"constexpr\s+[\w ]+\s" + name + r"\s*=\s*([^;]+);", src).group(1).strip()
    assert const("kLazyMaxN") == "1024" and const("kLongSeg") == "32768" and const("kMaxDirect") == "2048" and const("kCk") == "8"
    assert const("kSincTileOutputs") == "1024" and "kForceEager = 8;" in src
    flags = {n: int(const(n)) for n in ("kFlagAmbiguous", "kFlagBadLength", "kFlagRange", "kFlagVerify", "kFlagDirectOverflow",
                                        "kFlagCkOverflow", "kFlagCapAmbiguous")}
    assert list(flags.values()) == [1, 2, 4, 8, 16, 32, 64]
    assert "zone = 1ull << 32" in src and "a >= 0x1p-11 && a < 0x1p62" in src
    fields = re.search(r"struct PlanHeader \{(.*?)\n\};", src, re.S).group(1)
    words, at = {}, 0
    for typ, field in re.findall(r"^\s*(int64_t|int32_t|double|unsigned long long)\s+(\w+);", fields, re.M):
        words[field] = at
        at += 1 if typ == "int32_t" else 2
    assert (words["cap"], words["flags"], words["n_direct"], words["n_long"], words["lazy"], words["lazy_fail"]) == \
        (P.H_CAP, P.H_FLAGS, P.H_N_DIRECT, P.H_N_LONG, P.H_LAZY, P.H_LAZY_FAIL)
