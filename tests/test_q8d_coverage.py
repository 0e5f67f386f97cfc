"""The case table of the small-batch layer's GPU tests (tests/qdecode_ref.py: cases(), run by tests/test_gpu_qdecode.py) reaches
every class it promises, checked on the CPU with the plan's Python restatement: every row count, every `in` (0 and every k
tail), forced split counts 1 - 3 wherever no range is empty -- uneven last ranges and a last range that holds only a k tail among
them --, every out (a thin last strip, several strips), both weight kinds, every x pitch and base, wide and single stores of
both outputs, all four epilogues.  A change that drops a class from the table fails here, without a GPU.  The second table
(wide_deep_cases()) is held to what the first stops short of: more than one finish workgroup per row, more than three K ranges up
to one per slice, ranges of 33, 43 and 86 slices, every row count from 1 to 16.

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


# ---- the second table (D.wide_deep_cases(), run by tests/test_gpu_qdecode.py too): what the first one stops short of ---------
WIDE = D.wide_deep_cases()


def _plans(c, cus=256):
    """(the fp32 call's plan, the int8 call's) of a case on its own output layouts."""
    (ypad, yoff), (qpad, qoff) = D.Y_LAYOUTS[c.y], D.YQ_LAYOUTS[c.yq]
    return (D.plan(c.rows, c.out, c.in_, False, c.out + ypad, 4 * yoff % 16, c.splits, cus),
            D.plan(c.rows, c.out, c.in_, True, c.out + qpad, qoff % 16, c.splits, cus))


def _finish_x(c):
    return -(-c.out // D.FINISH_COLS)


def test_the_second_table_is_new_and_every_case_has_a_plan():
    ids = [D.case_id(c) for c in WIDE]
    assert len(set(ids)) == len(ids) and not set(ids) & {D.case_id(c) for c in CASES}
    for c in WIDE:
        assert all(p is not None for p in _plans(c)), c
        assert c.in_ > 0 and 1 <= c.rows <= D.MAX_ROWS
    assert {c.weight for c in WIDE} == {"qweight", "image"} and {(c.bias, c.relu) for c in WIDE} == set(D.EPILOGUES)
    assert {(c.x_pad, c.x_off) for c in WIDE} == set(D.X_LAYOUTS)


def test_the_finish_grid_of_the_second_table():
    """More than one finish workgroup per row: the blockIdx.x term of the finish kernel's column, and more than 3 strips."""
    assert D.WIDE_OUTS == (1024, 1025, 1027, 1028, 2049, 2177, 4100)
    grid = [c for c in WIDE if c.out in D.WIDE_OUTS and c.splits >= 2 and c.in_ in (129, 257, 385)]   # wide and shallow
    for out in D.WIDE_OUTS:
        assert len({c.rows for c in grid if c.out == out}) >= 2, out
    assert {_finish_x(c) for c in grid} == {1, 2, 3, 5}
    assert {-(-c.out // D.STRIP) for c in grid} == {8, 9, 17, 18, 33}
    assert {c.out - (c.out - 1) // D.STRIP * D.STRIP for c in grid} >= {1, 3, 4, 128}   # columns of the last strip
    assert {c.out - (_finish_x(c) - 1) * D.FINISH_COLS for c in grid} >= {1, 3, 4, 129, 1024}   # ... of the last finish workgroup
    assert {c.splits for c in grid} >= {2, 3, 4}
    # the stores' forms where blockIdx.x > 0 exists: wide and single of both outputs, and wide ones of an out that is no multiple
    # of 4 (the row's last columns leave one by one, from the LAST workgroup)
    for out8 in (False, True):
        forms = {("wide" in _plans(c)[out8][0], c.out % 4 != 0) for c in grid if _finish_x(c) >= 2}
        assert forms >= {(True, True), (True, False), (False, True), (False, False)}, (out8, forms)


def test_the_range_counts_of_the_second_table():
    """Forced counts above 3 up to one range per slice, and the plan's own choice where every slice has its own workgroup."""
    for in_ in D.MANY_RANGES_INS:
        slices = -(-in_ // D.SLICE)
        valid = {s for s in range(4, slices + 1) if D.valid_splits(in_, s)}
        assert {c.splits for c in WIDE if c.in_ == in_ and c.splits > 3} == valid >= {5, slices}, (in_, valid)
    assert D.MANY_RANGES_INS == (1153, 1280)
    lasts = {(c.in_, c.splits): D.ranges(c.in_, c.splits)[1][-1] for c in WIDE if c.in_ in D.MANY_RANGES_INS}
    assert lasts[1153, 10] == (1152, 1153) and lasts[1280, 10] == (1152, 1280)   # the one-byte tail alone; an even split
    assert lasts[1153, 5] == (1024, 1153) and D.ranges(1153, 5)[0] == 256        # an uneven last range: a slice and the tail
    own = [c for c in WIDE if c.splits == 0]
    assert {(c.rows, c.out, c.in_) for c in own} == set(D.OWN_CHOICE) == {(1, 130, 8192), (2, 130, 8192), (1, 1025, 4224)}
    got = {(c.rows, c.out, c.in_): _plans(c)[0][2:] for c in own}
    assert got == {(1, 130, 8192): (64, 128), (2, 130, 8192): (64, 128), (1, 1025, 4224): (33, 128)}
    assert any(_plans(c)[0][2] == -(-c.in_ // D.SLICE) for c in own), "no own choice of one slice per range at 256 CUs"
    assert any(_plans(c)[0][2] == -(-c.in_ // D.SLICE) and _finish_x(c) >= 2 for c in own)
    # the finish loop's s goes far past the first table's 15 (own choice) and 2 (forced)
    assert max(_plans(c)[0][2] for c in WIDE) == 64 and max(c.splits for c in WIDE) == 10
    assert max(c.splits for c in CASES) == 3


def test_the_range_depths_of_the_second_table():
    """Slices per range: the two-stage ring goes round 17, 22 and 43 times (the first table: five)."""
    deep = {(c.in_, c.splits): c for c in WIDE if c.rows == D.MAX_ROWS and c.out == 130 and c.in_ >= 4224}
    assert set(deep) == set(D.DEEP) == {(4224, 1), (11008, 1), (11008, 2)}
    assert {k: D.ranges(*k)[0] // D.SLICE for k in deep} == {(4224, 1): 33, (11008, 1): 86, (11008, 2): 43}
    assert {c.weight for c in deep.values()} == {"qweight", "image"}
    assert max(D.ranges(c.in_, c.splits)[0] // D.SLICE for c in CASES if c.splits) == 10
    # an odd slice count: the last ring round is one real slice and one zero slice; an even one: both real
    assert {D.ranges(*k)[0] // D.SLICE % 2 for k in deep} == {0, 1}


def test_every_row_count_of_the_second_table():
    out, in_, splits = D.LADDER
    ladder = [c for c in WIDE if (c.out, c.in_, c.splits) == (130, 257, 2)]
    assert (out, in_, splits) == (130, 257, 2) and [c.rows for c in ladder] == list(range(1, 17))
    assert len({(c.x_pad, c.x_off) for c in ladder}) == 16 and {c.weight for c in ladder} == {"qweight", "image"}
    assert {c.y for c in ladder} == set(range(len(D.Y_LAYOUTS))) and {c.yq for c in ladder} == set(range(len(D.YQ_LAYOUTS)))


def test_the_reserved_workspaces_shape_has_a_split_count_that_varies_with_the_rows():
    """tests/test_gpu_qdecode.py's reserve_decode() test: the plan's own count differs between row counts, and the largest
    workspace is not the one of 16 rows -- a reserve_decode() that planned 16 rows alone would be too small."""
    out, in_ = D.RESERVE_SHAPE
    for cus in (256, 304, 64):
        plans = {rows: D.plan(rows, out, in_, cus=cus) for rows in range(1, D.MAX_ROWS + 1)}
        assert len({p[2] for p in plans.values()}) >= 4, cus
        assert max(p[1] for p in plans.values()) > plans[D.MAX_ROWS][1], cus
    assert D.valid_splits(in_, 3)


@built_lib.needs_library
def test_the_librarys_plan_says_the_same_of_every_case():
    if not built_lib.library_loads():
        pytest.skip("libmmult_hip_q8d.so (or the HIP runtime it links) is not loadable here")
    from how_to_optimize_gemm_amd import q8
    for c in CASES + WIDE:
        for out8, (pad, off) in ((False, D.Y_LAYOUTS[c.y]), (True, D.YQ_LAYOUTS[c.yq])):
            o16 = (off * (1 if out8 else 4)) % 16
            ldq = (((c.in_ + 3) & ~3) + c.x_pad) if c.in_ else c.x_pad
            got = q8.qlinear_decode_plan(c.rows, c.out, c.in_, ldq=ldq, out8=out8, ldo=c.out + pad, o_mod16=o16, splits=c.splits, cu_count=256)
            assert got == D.plan(c.rows, c.out, c.in_, out8, c.out + pad, o16, c.splits, 256)[:2], c


# ---- the inputs' host-side conditions ---------------------------------------------------------------------------------------
def test_every_slice_of_k_moves_the_sums_of_every_case(oracle):
    """problem() and image_problem() assert their conditions themselves; here they run on the CPU for every shape of the table."""
    for c in CASES + WIDE:
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
