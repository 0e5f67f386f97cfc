"""The case table of the small-batch layer's GPU tests (tests/qdecode_ref.py: cases(), run by tests/test_gpu_qdecode.py) reaches
every class it promises, checked on the CPU with the plan's Python restatement: every row count, every `in` (0 and every k
tail), forced split counts 1 - 3 wherever no range is empty -- uneven last ranges and a last range that holds only a k tail among
them --, every out (a thin last strip, several strips), both weight kinds, every x pitch and base, wide and single stores of
both outputs, all four epilogues.  A change that drops a class from the table fails here, without a GPU.

Also here, because they need no GPU either: the host-side conditions of that module's inputs."""
import pytest

import built_lib
import qdecode_ref as D

CASES = D.cases()


def test_the_table_has_every_row_count_in_and_out():
    assert len(set(CASES)) == len(CASES) and len({D.case_id(c) for c in CASES}) == len(CASES)
    assert {c.rows for c in CASES} == set(D.ROWS) == {1, 2, 15, 16}
    assert {c.in_ for c in CASES} == set(D.INS) == {0, 1, 63, 64, 65, 127, 128, 129, 384, 385, 1153}
    assert {c.out for c in CASES} >= set(D.OUTS) == {1, 16, 17, 127, 128, 129, 257, 271, 273}
    # every out at two row counts behind at least two K ranges; in == 0 at every row count
    for out in D.OUTS:
        assert len({c.rows for c in CASES if c.out == out and c.splits >= 2}) >= 2, out
    assert {c.rows for c in CASES if c.in_ == 0} == set(D.ROWS)
    assert all(c.splits == 0 and c.weight == "image" for c in CASES if c.in_ == 0)


def test_forced_splits_wherever_no_range_is_empty():
    for in_ in D.INS[1:]:
        for s in D.FORCED:
            have = any(c.in_ == in_ and c.splits == s for c in CASES)
            assert have == D.valid_splits(in_, s), (in_, s)
            assert (D.plan(16, 128, in_, splits=s) is not None) == D.valid_splits(in_, s)
    assert all(c.splits in D.FORCED for c in CASES if c.in_)
    lasts = set()
    for c in CASES:
        if c.splits >= 2:
            k_len, rs = D.ranges(c.in_, c.splits)
            assert all(b < e for b, e in rs)
            lasts.add((rs[-1][1] - rs[-1][0], k_len))
    assert any(last == 1 for last, _ in lasts), "no last range that holds only a one-byte k tail"
    assert any(1 < last < k_len and last % 128 == 0 for last, k_len in lasts), "no uneven last range of whole slices"
    assert any(last % 128 not in (0, 1) or (last > 128 and last % 128 == 1) for last, _ in lasts), "no last range of slices and a tail"
    assert any(last == k_len for last, k_len in lasts), "no even split"
    # several slices per range too: the ring goes round
    assert any(D.ranges(c.in_, c.splits)[0] >= 512 for c in CASES if c.splits)


def test_strips_layouts_weights_and_epilogues():
    strips = {-(-c.out // D.STRIP) for c in CASES}
    assert strips == {1, 2, 3}
    assert {c.out - 2 * D.STRIP for c in CASES if c.out > 2 * D.STRIP} == {1, 15, 17}      # a thin last strip behind two whole ones
    assert {(c.x_pad, c.x_off) for c in CASES if c.in_} == set(D.X_LAYOUTS) and len(D.X_LAYOUTS) == 16
    assert {c.y for c in CASES} == set(range(len(D.Y_LAYOUTS))) and {c.yq for c in CASES} == set(range(len(D.YQ_LAYOUTS)))
    for c in CASES:
        for out8, (pad, off) in ((False, D.Y_LAYOUTS[c.y]), (True, D.YQ_LAYOUTS[c.yq])):
            assert D.plan(c.rows, c.out, c.in_, out8, c.out + pad, (off * (1 if out8 else 4)) % 16, c.splits) is not None, c
    wide = lambda c, out8: "wide" in D.plan(c.rows, c.out, c.in_, out8, c.out + (D.YQ_LAYOUTS[c.yq] if out8 else D.Y_LAYOUTS[c.y])[0],
                                            ((D.YQ_LAYOUTS[c.yq][1]) if out8 else 4 * D.Y_LAYOUTS[c.y][1]) % 16, c.splits)[0]
    for out8 in (False, True):
        assert {wide(c, out8) for c in CASES} == {False, True}, out8
        # wide stores meet an out that is no multiple of 4 (the row's last columns leave one by one) and one that is
        assert any(wide(c, out8) and c.out % 4 for c in CASES) and any(wide(c, out8) and c.out % 4 == 0 for c in CASES), out8
    assert any(D.Y_LAYOUTS[c.y][0] % 2 for c in CASES) and {D.YQ_LAYOUTS[c.yq][1] for c in CASES} >= {1, 2, 3}
    assert any((c.out + D.YQ_LAYOUTS[c.yq][0]) % 2 for c in CASES)
    assert {c.weight for c in CASES if c.in_} == {"qweight", "image"}
    assert {(c.bias, c.relu) for c in CASES} == set(D.EPILOGUES) and len(set(D.EPILOGUES)) == 4
    for kind in ("qweight", "image"):
        assert {c.splits for c in CASES if c.weight == kind and c.in_} == {1, 2, 3}, kind


def test_the_plans_own_choice_splits_at_the_mi355x():
    text, work, splits, k_len = D.plan(*D.PLAN_SHAPE, cus=256)
    assert splits == 16 and k_len == 512 and work == D.work_bytes(16, 16, 256), text
    assert D.plan(*D.PLAN_SHAPE, cus=8)[2] < splits


@built_lib.needs_library
def test_the_librarys_plan_says_the_same_of_every_case():
    if not built_lib.library_loads():
        pytest.skip("libmmult_hip_q8d.so (or the HIP runtime it links) is not loadable here")
    from how_to_optimize_gemm_amd import q8
    for c in CASES:
        for out8, (pad, off) in ((False, D.Y_LAYOUTS[c.y]), (True, D.YQ_LAYOUTS[c.yq])):
            o16 = (off * (1 if out8 else 4)) % 16
            ldq = (((c.in_ + 3) & ~3) + c.x_pad) if c.in_ else c.x_pad
            got = q8.qlinear_decode_plan(c.rows, c.out, c.in_, ldq=ldq, out8=out8, ldo=c.out + pad, o_mod16=o16, splits=c.splits, cu_count=256)
            assert got == D.plan(c.rows, c.out, c.in_, out8, c.out + pad, o16, c.splits, 256)[:2], c


# ---- the inputs' host-side conditions ---------------------------------------------------------------------------------------
def test_every_slice_of_k_moves_the_sums_of_every_case(oracle):
    """problem() and image_problem() assert their conditions themselves; here they run on the CPU for every shape of the table."""
    for c in CASES:
        p = (D.problem if c.weight == "qweight" else D.image_problem)(c.rows, c.out, c.in_)
        assert p.acc.shape == (c.rows, c.out) and (c.in_ == 0) == (not p.acc.any())
    D.problem(15, 2 * D.STRIP + 17, 385)
    D.image_problem(16, 2 * D.STRIP + 15, 385)


def test_a_slice_that_does_not_move_the_sums_is_noticed(oracle):
    import qlinear_ref as R
    p = D.problem(16, 129, 385)
    dead = p.xq.copy()
    dead[:, 128:256] = 0
    with pytest.raises(AssertionError):
        D.every_slice_moves_the_sums(dead, p.qw, R.int_sums(dead, p.qw))


def test_the_large_sums_are_what_their_test_says(oracle):
    p = D.large_sums_problem()
    assert p.xq.shape == (16, 2048) and D.valid_splits(2048, 4) and D.ranges(2048, 4)[0] == 512
