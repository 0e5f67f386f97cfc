"""The case table of the 4-bit layer's GPU tests (tests/q4_ref.py: cases(), run by tests/test_gpu_q4decode.py) reaches every
class it promises, checked on the CPU with the plan's Python restatement: every row count, every `in` -- every position of the
k tail relative to a slice's low half, its high half and the slice boundary --, every out, forced split counts 1 - 3 wherever no
range is empty with uneven and one-slice last ranges among them, both weight kinds, every x pitch and base, wide and single
stores of both outputs, all four epilogues.  A change that drops a class from the table fails here, without a GPU.

Also here, because they need no GPU either: the host-side conditions of that module's inputs."""
import numpy as np
import pytest

import built_lib
import q4_ref as F
import qdecode_ref as D

CASES = F.cases()


def test_the_table_has_every_row_count_in_and_out():
    assert len(set(CASES)) == len(CASES) and len({F.case_id(c) for c in CASES}) == len(CASES)
    assert {c.rows for c in CASES} == set(F.ROWS) == {1, 2, 15, 16}
    assert {c.in_ for c in CASES} == set(F.INS) == {1, 63, 64, 65, 127, 128, 129, 384, 385, 1153}
    assert {c.out for c in CASES} == set(F.OUTS) == {1, 16, 17, 127, 128, 129, 257, 273}
    for out in F.OUTS:
        assert len({c.rows for c in CASES if c.out == out and c.splits >= 2}) >= 2, out
    # the tail of the last slice: inside the low half, exactly the low half, one into the high half, inside it, a whole slice
    tails = {(c.in_ - 1) % 128 + 1 for c in CASES}
    assert tails >= {1, 63, 64, 65, 127, 128}
    assert {-(-c.in_ // 128) for c in CASES} >= {1, 2, 3, 4, 10}


def test_forced_splits_wherever_no_range_is_empty():
    for in_ in F.INS:
        for s in F.FORCED:
            have = any(c.in_ == in_ and c.splits == s for c in CASES)
            assert have == D.valid_splits(in_, s), (in_, s)
            assert (F.plan(16, 128, in_, splits=s) is not None) == D.valid_splits(in_, s)
    assert all(c.splits in F.FORCED for c in CASES)
    lasts = set()
    for c in CASES:
        if c.splits >= 2:
            k_len, rs = D.ranges(c.in_, c.splits)
            assert all(b < e for b, e in rs)
            lasts.add((rs[-1][1] - rs[-1][0], k_len))
    assert any(last == 1 for last, _ in lasts), "no last range that holds only a one-byte k tail"
    assert any(last <= 128 < k_len for last, k_len in lasts), "no one-slice last range behind longer ones"
    assert any(1 < last < k_len and last % 128 == 0 for last, k_len in lasts), "no uneven last range of whole slices"
    assert any(last == k_len for last, k_len in lasts), "no even split"
    assert any(D.ranges(c.in_, c.splits)[0] >= 512 for c in CASES), "the ring never goes round"


def test_strips_layouts_weights_and_epilogues():
    assert {-(-c.out // F.STRIP) for c in CASES} == {1, 2, 3}
    assert {(c.x_pad, c.x_off) for c in CASES} == set(D.X_LAYOUTS) and len(D.X_LAYOUTS) == 16
    assert {c.y for c in CASES} == set(range(len(D.Y_LAYOUTS))) and {c.yq for c in CASES} == set(range(len(D.YQ_LAYOUTS)))

    def planned(c, out8):
        pad, off = (D.YQ_LAYOUTS[c.yq] if out8 else D.Y_LAYOUTS[c.y])
        return F.plan(c.rows, c.out, c.in_, out8, c.out + pad, (off * (1 if out8 else 4)) % 16, c.splits)

    for out8 in (False, True):
        assert all(planned(c, out8) not in (None, "long") for c in CASES)
        assert {"wide" in planned(c, out8)[0] for c in CASES} == {False, True}, out8
        assert any("wide" in planned(c, out8)[0] and c.out % 4 for c in CASES), out8
    assert {c.weight for c in CASES} == {"qweight", "image"}
    assert {(c.bias, c.relu) for c in CASES} == set(D.EPILOGUES) and len(set(D.EPILOGUES)) == 4
    for kind in ("qweight", "image"):
        assert {c.splits for c in CASES if c.weight == kind} == {1, 2, 3}, kind
        # a last slice that ends inside its low half, inside its high half, and a whole one
        tails = {(c.in_ - 1) % 128 + 1 for c in CASES if c.weight == kind}
        assert {"low" if t <= 64 else "high" if t < 128 else "whole" for t in tails} == {"low", "high", "whole"} and 1 in tails, kind


def test_the_plans_own_choice_and_the_deep_case():
    text, work, splits, k_len = F.plan(*F.PLAN_SHAPE, cus=256)
    assert splits == 8 and k_len == 1024 and work == D.work_bytes(8, 16, 256), text   # (the int8 plan: 16 of 512 -- half the bytes)
    assert F.plan(*F.PLAN_SHAPE, cus=8)[2] < splits
    rows, out, in_, s = F.DEEP
    assert F.plan(rows, out, in_, splits=s)[2:] == (1, 11008) and max(D.ranges(c.in_, c.splits)[0] for c in CASES) < 11008


@built_lib.needs_library
def test_the_librarys_plan_says_the_same_of_every_case():
    if not built_lib.library_loads():
        pytest.skip("libmmult_hip_q4d.so (or the HIP runtime it links) is not loadable here")
    from how_to_optimize_gemm_amd import q8
    for c in CASES:
        for out8, (pad, off) in ((False, D.Y_LAYOUTS[c.y]), (True, D.YQ_LAYOUTS[c.yq])):
            o16 = (off * (1 if out8 else 4)) % 16
            ldq = ((c.in_ + 3) & ~3) + c.x_pad
            got = q8.qlinear_decode4_plan(c.rows, c.out, c.in_, ldq=ldq, out8=out8, ldo=c.out + pad, o_mod16=o16, splits=c.splits, cu_count=256)
            assert got == F.plan(c.rows, c.out, c.in_, out8, c.out + pad, o16, c.splits, 256)[:2], c


# ---- the inputs' host-side conditions ---------------------------------------------------------------------------------------
def test_every_half_slice_moves_the_sums_of_every_case():
    """problem() and image_problem() assert their conditions themselves; here they run on the CPU for every shape the GPU module
    uses.  Library-made weights never hold -8; caller-made images hold every value in both nibble positions."""
    for c in CASES:
        p = (F.problem if c.weight == "qweight" else F.image_problem)(c.rows, c.out, c.in_)
        assert p.acc.shape == (c.rows, c.out) and p.acc.any()
        assert (p.W.min() >= -7) == (c.weight == "qweight") or p.W.size < 64, c
    for rows, out, in_ in ((15, 273, 385), (2, 129, 129), (16, 273, 1153), (15, 273, 1153), F.PLAN_SHAPE, F.DEEP[:3]):
        F.problem(rows, out, in_)
    big = F.image_problem(16, 271, 385)
    assert set(np.unique(big.W)) == set(range(-8, 8)) and (big.xq == -128).any()
    for shape in F.EQUAL_SHAPES:
        F.image_problem(*shape)


def test_a_half_that_does_not_move_the_sums_or_equals_its_neighbour_is_noticed():
    p = F.problem(16, 129, 385)
    dead = p.xq.copy()
    dead[:, 192:256] = 0                               # the high half of the second slice
    with pytest.raises(AssertionError):
        F.every_half_slice_moves_the_sums(dead, p.W, F.int_sums(dead, p.W))
    twin = p.W.copy()
    twin[64:128] = twin[:64]                           # a slice whose halves could be swapped unseen
    with pytest.raises(AssertionError):
        F.every_half_slice_moves_the_sums(p.xq, twin, F.int_sums(p.xq, twin))


def test_the_large_sums_are_what_their_test_says():
    p = F.large_sums_problem()
    assert p.xq.shape == (16, 24576) and D.valid_splits(24576, 4) and D.ranges(24576, 4)[0] == 6144 <= F.MAX_RANGE_K
    assert np.abs(p.acc).max() > 1 << 24 and set(np.unique(p.W)) == {-8, 7}
