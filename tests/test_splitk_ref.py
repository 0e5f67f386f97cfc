"""tests/splitk_ref.py, the restatement of the split-K kernels' bit contract, checked on the CPU: one part is the chain,
integer-valued inputs are exact for every part count, the boundaries are floor(nk s / S) -- and the condition that gives the
GPU table (tests/test_gpu_splitk_parity.py) its teeth: at every shape and part count it runs, the restated bits differ from the
chain's, from those of S - 1 and S + 1 parts and from "C added behind the fold" in a large share of the elements.  The shares
are conditions on the reference; nothing here has seen a kernel's output."""
import functools
import os

import numpy as np
import pytest

import splitk_ref as ref
import test_gpu_splitk_parity as T

CUS = 256   # the MI355X's compute units (the GPU test derives its part counts from the device's count)
KB = T.KB


def test_one_part_is_the_chain(oracle):
    a, b, c0 = T.inputs(128, 64, 224)
    assert np.array_equal(ref.splitk_ref(oracle, a, b, None, 1).view(np.uint32), oracle.ref_mmult(a, b, fma=True).view(np.uint32))
    assert np.array_equal(ref.splitk_ref(oracle, a, b, c0, 1).view(np.uint32), oracle.ref_mmult(a, b, c0.copy(), fma=True).view(np.uint32))
    assert np.array_equal(ref.c_added_last(oracle, a, b, c0, 1), oracle.ref_mmult(a, b, fma=True) + c0)


def test_integer_valued_inputs_are_exact_for_every_part_count(oracle):
    m, n, k = 128, 128, 224
    a, b = oracle.harness_inputs(m, n, k, pattern=3)
    exact = a.astype(np.float64) @ b.astype(np.float64)
    c0 = np.arange(m * n, dtype=np.float32).reshape(m, n) % 5
    for S in range(1, k // KB + 1):
        assert np.array_equal(ref.splitk_ref(oracle, a, b, None, S).astype(np.float64), exact), S
        assert np.array_equal(ref.splitk_ref(oracle, a, b, c0, S).astype(np.float64), exact + c0), S


def test_boundaries_and_counts():
    assert ref.boundaries(7, 4) == [0, 1, 3, 5, 7]
    assert ref.boundaries(3, 2) == [0, 1, 3] and ref.boundaries(3, 3) == [0, 1, 2, 3] and ref.boundaries(8, 5) == [0, 1, 3, 4, 6, 8]
    for nk in range(1, 70):
        for S in range(1, nk + 1):
            cut = ref.boundaries(nk, S)
            assert cut[0] == 0 and cut[-1] == nk and all(x < y for x, y in zip(cut, cut[1:])), (nk, S)   # no part is empty
    assert ref.parts_launched(8, 3) == 3 and ref.parts_launched(2, 3) == 2 and ref.parts_launched(4, 1) == 1
    # policy.hip splitk_auto_parts: min(2 cus / tiles, k / 256, 8)
    assert [ref.auto_parts(256, 1, k) for k in (224, 256, 512, 1024, 2048, 4096)] == [0, 1, 2, 4, 8, 8]
    assert ref.auto_parts(256, 64, 2048) == 8 and ref.auto_parts(256, 100, 2048) == 5 and ref.auto_parts(256, 300, 2048) == 1
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "how-to-optimize-gemm_amd", "csrc", "policy.hip")).read()
    assert "const int S = (int)((2 * cus) / (tiles > 0 ? tiles : 1));" in src and "return std::min(std::min(S, k / (8 * kSliceK)), 8);" in src


def test_the_parts_of_a_restatement_are_the_contracts(oracle):
    """Part s on its own: the chain over its K range, from zero (from C: part 0 only), and the fold in part order."""
    a, b, c0 = T.inputs(128, 64, 224)
    ps = ref.partials(oracle, a, b, c0, 4)
    cut = [0, 32, 96, 160, 224]
    for s in range(4):
        start = c0.copy() if s == 0 else None
        want = oracle.ref_mmult(np.ascontiguousarray(a[:, cut[s]:cut[s + 1]]), np.ascontiguousarray(b[cut[s]:cut[s + 1]]), start, fma=True)
        assert np.array_equal(ps[s].view(np.uint32), want.view(np.uint32)), s
    assert np.array_equal(ref.fold(ps), ((ps[0] + ps[1]) + ps[2]) + ps[3])
    assert ref.differing_share(ref.fold(ps), ref.fold(ps, descending=True)) >= 0.25     # the order of the fold is part of the bits


# ---- the condition that gives the GPU table its teeth -----------------------------------------------------------------
def table_points():
    """(m, n, k, seed, S) of every launch of the GPU module: the table's cases at the restated part count (a residency case:
    every count the clamp can leave), the special-value tile aside, and the shared shape at the counts its tests run."""
    points = set()
    for row in T.SPLITK_INSTANTIATIONS:
        bm, bn, _ = row.tile
        for case in row.cases(CUS):
            tile = (128, 128) if case.auto else (bm, bn)
            S = T.expected_parts(case, *tile, CUS)
            left = T.residency_counts(*tile, CUS, (case.m // bm) * (case.n // bn)) if case.residency else (S,)
            assert all(2 <= s <= S for s in left) and (not case.residency or max(left) < S == 8), (row.symbol, case, left)
            for s in left:
                points.add((case.m, case.n, case.k, 0, s))
    m, n, k = T.SHARED_SHAPE
    points |= {(m, n, k, 1, 4), (m, n, k, 2, 4), (m, n, k, 3, 2), (m, n, k, 4, 4), (m, n, k, 5, 4), (m, n, k, 6, 4), (m, n, k, 8, 4), (m, n, k, 9, 4)}
    return sorted(points)


@functools.lru_cache(maxsize=None)
def _restated(m, n, k, seed, S):
    """(overwrite, accumulate, C added last) at S parts; S = 1 is the chain."""
    a, b, c0 = T.inputs(m, n, k, seed)
    over, acc = T.restated(a, b, c0, S)
    return over, acc, over + c0


def test_the_table_runs_the_cases_the_contract_can_fail_at():
    points = table_points()
    assert {(128, 128, 64, 0, 2), (128, 128, 96, 0, 2), (128, 128, 224, 0, 4), (128, 128, 96, 0, 3), (256, 384, 224, 0, 4),
            (128, 128, 512, 0, 2), (128, 128, 1024, 0, 4), (128, 128, 2048, 0, 8), (128, 64, 64, 0, 2), (256, 192, 224, 0, 4),
            (1280, 1280, 256, 0, 5), (1280, 640, 512, 0, 7)} <= set(points)


@pytest.mark.parametrize("m,n,k,seed,S", table_points())
def test_at_every_point_of_the_table_other_splits_give_other_bits(m, n, k, seed, S):
    nk = k // KB
    assert 2 <= S <= nk
    over, acc, c_last = _restated(m, n, k, seed, S)
    share = ref.differing_share
    for other in (1, S - 1, S + 1):                  # the chain; one part fewer; one part more (where nk allows it)
        if other > nk or (other == S - 1 and other == 1):
            continue
        o_over, o_acc, _ = _restated(m, n, k, seed, other)
        assert share(over, o_over) >= 0.5, (other, share(over, o_over))
        assert share(acc, o_acc) >= 0.5, (other, share(acc, o_acc))
    assert share(acc, c_last) >= 0.25, share(acc, c_last)
