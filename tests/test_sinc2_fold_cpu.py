"""The folded third K slice of the streaming kernel's banks (csrc/sinc2.hip, r11), without a GPU:
  * the two new header tables are the model's folded fragments (tools/sinc2_model.py), and every slice-2 fragment the fold rests
    on is zero in lanes 16-63;
  * a float32-accumulated emulation of the folded rows against the unfolded ones, every sub-position, full-range and small input;
  * MFMAs per iteration of the mono hot loops, from the compiler's listing (tools/isa_census.py).

Bound of the emulation.  Both forms sum the same exact float16 products in float32, in another order: the unfolded rows' own
distance from the float64 sum of those products is measured in the same test, and the folded rows may lie twice that from
them (the two forms' rounding errors are independent and of that size each)."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LO = 4096.0


def _header_table(name):
    text = open(os.path.join(ROOT, "pyaudiorestoration_amd", "csrc", "sinc_taps_gen.h")).read()
    body = text[text.index(name + "["):]
    body = body[body.index("{") + 1:body.index("};")]
    return np.array([int(h, 16) for h in re.findall(r"0x([0-9a-f]{8})u", body)], dtype=np.uint32)


def _words(frag):
    fr = frag.reshape(-1, 2)
    return fr[:, 0].astype(np.uint32) | (fr[:, 1].astype(np.uint32) << 16)


def test_fold_fragments_in_the_header_are_the_models():
    import sinc2_model as M2
    for name, frag in (("kBank2FoldFrag32", M2.bank_fold_fragment()), ("kBank3FoldFrag32", M2.moment_fold_fragment())):
        have = _header_table(name)
        assert frag.shape == (64, 8) and have.shape == (256,) and np.array_equal(have, _words(frag)), name
    # the tables the fold leaves as they are
    assert np.array_equal(_header_table("kBank2Frags32"), _words(M2.bank_fragments()))
    assert np.array_equal(_header_table("kBank3Frags32"), _words(M2.moment_fragments()))


def test_slice_2_lives_in_k_group_0():
    """what the fold rests on: every slice-2 fragment is zero in lanes 16-63, its elements sit at j <= i - 2; the folded
    fragments hold the pair's hi slice x 4096 (exactly), its lo slice, its hi slice and zeros"""
    import sinc2_model as M2
    for frags, table, hi, lo, fold in ((M2.bank_fragments(), M2.FRAGS, 2, 7, M2.bank_fold_fragment()),
                                       (M2.moment_fragments(), M2.MOM_FRAGS, 2, 5, M2.moment_fold_fragment())):
        f = frags.view(np.float16).astype(np.float64)
        for k in M2.slice2_fragments(table):
            assert not f[k, 16:].any(), k
            for m in range(16):
                i = m >> 1
                assert not f[k, m, max(i - 1, 0):].any(), (k, m)
        v = fold.view(np.float16).astype(np.float64)
        assert np.array_equal(v[:16], LO * f[hi, :16]) and np.array_equal(v[16:32], f[lo, :16])
        assert np.array_equal(v[32:48], f[hi, :16]) and not v[48:].any()
        assert np.max(np.abs(v)) < 65504.0


def _mfma(acc, A, B):
    """acc[m][n] += sum_k A[m][k] B[k][n]: exact float16 products (22 significant bits), accumulated in float32 in K order"""
    for k in range(A.shape[1]):
        acc = (acc + (A[:, k:k + 1].astype(np.float32) * B[k:k + 1, :].astype(np.float32))).astype(np.float32)
    return acc


def _a_matrix(frag):
    """[16 rows m][32 K entries] of one constant fragment [64 lanes][8]: lane = m + 16 g, K = 8 g + j"""
    f = frag.view(np.float16).reshape(4, 16, 8)
    return np.concatenate([f[g] for g in range(4)], axis=1)


@pytest.mark.parametrize("scale", [32.0, 1e-3])
@pytest.mark.parametrize("pair", ["bank", "moments"])
def test_folded_rows_against_unfolded_rows(pair, scale):
    """v0 = e0 + lo 2^-12 (and m01 likewise) of 16 blocks x 8 sub-positions, both ways, against the float64 sum"""
    import sinc2_model as M2
    if pair == "bank":
        fr, fold, hi_f, lo_f = M2.bank_fragments(), M2.bank_fold_fragment(), (0, 1, 2), (5, 6, 7)
    else:
        fr, fold, hi_f, lo_f = M2.moment_fragments(), M2.moment_fold_fragment(), (0, 1, 2), (3, 4, 5)
    rng = np.random.default_rng(5)
    worst_own, worst_fold, peak = 0.0, 0.0, 0.0
    for trial in range(4):
        x = rng.uniform(-scale, scale, 16 * 8 + 96) * 1024.0                  # the images hold the signal x 1024
        xh, xl = M2.split16(x)
        xh16, xl16 = xh.astype(np.float16), xl.astype(np.float16)
        # B[k][bb] = image[8 bb + k], k = 0 .. 95
        Bh = np.stack([xh16[8 * bb:8 * bb + 96] for bb in range(16)], axis=1)
        Bl = np.stack([xl16[8 * bb:8 * bb + 96] for bb in range(16)], axis=1)
        Ah = [_a_matrix(fr[k]) for k in hi_f]
        Al = [_a_matrix(fr[k]) for k in lo_f]
        z = np.zeros((16, 16), dtype=np.float32)
        # unfolded: three slices each
        e0, lo = z, z
        for ks in range(3):
            sl = slice(32 * ks, 32 * ks + 32)
            e0 = _mfma(e0, Ah[ks], Bh[sl])
            lo = _mfma(lo, Al[ks], Bh[sl])
            lo = _mfma(lo, Ah[ks], Bl[sl])
        unfolded = (e0 + lo * np.float32(1.0 / LO)).astype(np.float32)
        # folded: two slices, then V x xv (K groups: hi image, hi image, lo image, hi image, all at K entries 64 .. 71)
        e0, lo = z, z
        for ks in range(2):
            sl = slice(32 * ks, 32 * ks + 32)
            e0 = _mfma(e0, Ah[ks], Bh[sl])
            lo = _mfma(lo, Al[ks], Bh[sl])
            lo = _mfma(lo, Ah[ks], Bl[sl])
        xv = np.concatenate([Bh[64:72], Bh[64:72], Bl[64:72], Bh[64:72]], axis=0)
        lo = _mfma(lo, _a_matrix(fold), xv)
        folded = (e0 + lo * np.float32(1.0 / LO)).astype(np.float32)
        # the exact sum of the same products
        exact = np.zeros((16, 16))
        for ks in range(3):
            sl = slice(32 * ks, 32 * ks + 32)
            exact += Ah[ks].astype(np.float64) @ Bh[sl].astype(np.float64)
            exact += (Al[ks].astype(np.float64) @ Bh[sl].astype(np.float64) + Ah[ks].astype(np.float64) @ Bl[sl].astype(np.float64)) / LO
        peak = max(peak, float(np.max(np.abs(exact))))
        worst_own = max(worst_own, float(np.max(np.abs(unfolded - exact))))
        worst_fold = max(worst_fold, float(np.max(np.abs(folded.astype(np.float64) - unfolded))))
    print(f"{pair} |x| <= {scale}: unfolded rows {worst_own / peak:.2e} of the rows' peak from the float64 sum, folded rows "
          f"{worst_fold / peak:.2e} from the unfolded ones")
    assert worst_own > 0.0
    assert worst_fold <= 2.0 * worst_own, (pair, scale, worst_fold, worst_own)


def test_the_fold_carries_the_overhang():
    """dropping V changes rows of sub-positions >= 2 (and no others) by far more than rounding: the emulation above would
    see a fragment that missed the overhang"""
    import sinc2_model as M2
    fr, fold = M2.bank_fragments(), M2.bank_fold_fragment()
    x = np.random.default_rng(6).uniform(-1.0, 1.0, 16 * 8 + 96) * 1024.0
    xh, xl = M2.split16(x)
    Bh = np.stack([xh.astype(np.float16)[8 * bb:8 * bb + 96] for bb in range(16)], axis=1)
    Bl = np.stack([xl.astype(np.float16)[8 * bb:8 * bb + 96] for bb in range(16)], axis=1)
    xv = np.concatenate([Bh[64:72], Bh[64:72], Bl[64:72], Bh[64:72]], axis=0)
    over = _mfma(np.zeros((16, 16), dtype=np.float32), _a_matrix(fold), xv) / LO
    rows = np.max(np.abs(over), axis=1)                     # row m = 2 i + (e, d)
    assert not rows[:4].any() and np.all(rows[4:] > 1e-3), rows


@pytest.fixture(scope="module")
def census():
    spec = importlib.util.spec_from_file_location("isa_census", os.path.join(ROOT, "tools", "isa_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    L, files, stages = mod.compile_listing([])
    return mod, L, files, stages


@pytest.mark.parametrize("kind,want", [("2", [11, 24, 31]), ("1", [11])])
def test_mfmas_per_iteration(census, kind, want):
    mod, L, files, stages = census
    _, loops = mod.kernel_loops(L, "1", kind)
    have = sorted(mod.loop_totals(mod.loop_census(L, h, back, files, stages))["mfma"] for h, back in loops)
    assert have == want, (kind, have)
