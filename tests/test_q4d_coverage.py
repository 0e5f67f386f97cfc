"""The case table of the 4-bit layer's GPU tests (tests/q4_ref.py: cases(), run by tests/test_gpu_q4decode.py) reaches every
class it promises, checked on the CPU with the plan's Python restatement: every row count, every `in` -- every position of the
k tail relative to a slice's low half, its high half and the slice boundary --, every out, forced split counts 1 - 3 wherever no
range is empty with uneven and one-slice last ranges among them, both weight kinds, every x pitch and base, wide and single
stores of both outputs, all four epilogues.  A change that drops a class from the table fails here, without a GPU.  The second
table (wide_deep_cases()) is held to what the first stops short of: more than one finish workgroup per row, up to 33 strips,
more than three K ranges up to one per slice, ranges of 33 and 43 slices, every row count from 1 to 16; both tables together
to the ring's second stage, consumed as zeros or not, in last ranges and in others.

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


# ---- the second table (F.wide_deep_cases()): what the first one stops short of -------------------------------------------------
WIDE = F.wide_deep_cases()


def _plans(c, cus=256):
    """(fp32 plan, int8 plan) of a case on its own layouts."""
    got = []
    for out8, (pad, off) in ((False, D.Y_LAYOUTS[c.y]), (True, D.YQ_LAYOUTS[c.yq])):
        got.append(F.plan(c.rows, c.out, c.in_, out8, c.out + pad, (off * (1 if out8 else 4)) % 16, c.splits, cus))
    return got


def test_the_second_table_is_new_and_every_case_has_a_plan():
    ids = [F.case_id(c) for c in WIDE]
    assert 40 <= len(WIDE) <= 45 and len(set(ids)) == len(ids) and not set(ids) & {F.case_id(c) for c in CASES}
    for c in WIDE:
        assert all(p not in (None, "long") for p in _plans(c)), c
    assert {c.rows for c in WIDE} == set(range(1, F.MAX_ROWS + 1))
    assert {c.weight for c in WIDE} == {"qweight", "image"} and {(c.bias, c.relu) for c in WIDE} == set(D.EPILOGUES)
    assert {(c.x_pad, c.x_off) for c in WIDE} == set(D.X_LAYOUTS)
    for out8 in (0, 1):
        assert {"wide" in _plans(c)[out8][0] for c in WIDE} == {False, True}


def test_the_finish_grid_and_the_strips_of_the_second_table():
    """More than one finish workgroup per row -- the blockIdx.x term of the finish kernels' column, in THIS library's build of
    them -- and up to 33 strips of the partial kernel (the first table: 3)."""
    assert F.WIDE_OUTS == (1024, 1025, 1027, 1028, 2049, 2177, 4100)
    grid = [c for c in WIDE if c.out in F.WIDE_OUTS and c.splits >= 2]
    assert all(c.in_ <= 385 and 2 <= c.splits <= 4 for c in grid) and {c.splits for c in grid} == {2, 3, 4}
    for out in F.WIDE_OUTS:
        assert len({c.rows for c in grid if c.out == out}) >= 2, out
    assert {-(-c.out // D.FINISH_COLS) for c in grid} == {1, 2, 3, 5}
    assert {-(-c.out // F.STRIP) for c in grid} == {8, 9, 17, 18, 33} and max(-(-c.out // F.STRIP) for c in WIDE) >= 18
    odd = [c for c in WIDE if c.out == D.FINISH_COLS + 3]
    assert {(D.Y_LAYOUTS[c.y], D.YQ_LAYOUTS[c.yq]) for c in odd} >= {((1, 0), (5, 0))}
    for c in odd:
        if (D.Y_LAYOUTS[c.y], D.YQ_LAYOUTS[c.yq]) == ((1, 0), (5, 0)):
            assert all("wide stores" in p[0] for p in _plans(c)), c


def test_the_split_counts_of_the_second_table():
    """Every forced count above 3 that leaves no range empty, one range per slice among them; the plan's own choice where it is
    one slice per range at 256 CUs (every range then consumes a zero second stage)."""
    assert F.MANY_RANGES_INS == (1153, 1280)
    for in_ in F.MANY_RANGES_INS:
        slices = -(-in_ // F.SLICE)
        valid = {s for s in range(4, slices + 1) if D.valid_splits(in_, s)}
        assert {c.splits for c in WIDE if c.in_ == in_ and c.splits > 3} == valid >= {4, 5, slices}, (in_, valid)
    assert any(c.splits == -(-c.in_ // F.SLICE) and c.splits > 3 for c in WIDE), "no forced count equal to the slice count"
    own = [c for c in WIDE if c.splits == 0]
    assert {(c.rows, c.out, c.in_) for c in own} == set(F.OWN_CHOICE) == {(1, 130, 8192), (2, 130, 8192), (1, 1025, 4224)}
    got = {(c.rows, c.out, c.in_): _plans(c)[0][2:] for c in own}
    assert got == {(1, 130, 8192): (64, 128), (2, 130, 8192): (64, 128), (1, 1025, 4224): (33, 128)}
    assert max(_plans(c)[0][2] for c in WIDE) == 64 and max(c.splits for c in WIDE) == 10 and max(c.splits for c in CASES) == 3


def test_the_range_depths_and_the_ladder_of_the_second_table():
    deep = {(c.in_, c.splits): c for c in WIDE if c.rows == F.MAX_ROWS and c.out == 130 and c.in_ >= 4224}
    assert set(deep) == set(F.WIDE_DEEP) == {(4224, 1), (11008, 2)}
    assert {k: D.ranges(*k)[0] // F.SLICE for k in deep} == {(4224, 1): 33, (11008, 2): 43}
    assert {c.weight for c in deep.values()} == {"qweight", "image"}
    assert F.DEEP[2:] == (11008, 1)   # the 86 slices: the first module's own test
    ladder = [c for c in WIDE if (c.out, c.in_, c.splits) == F.LADDER]
    assert F.LADDER == (130, 257, 2) and [c.rows for c in ladder] == list(range(1, 17))
    assert len({(c.x_pad, c.x_off) for c in ladder}) == 16 and {c.weight for c in ladder} == {"qweight", "image"}
    assert {c.y for c in ladder} == set(range(len(D.Y_LAYOUTS))) and {c.yq for c in ladder} == set(range(len(D.YQ_LAYOUTS)))


def test_the_rings_second_stage_is_consumed_as_zeros_and_not_in_last_and_other_ranges():
    """Over every K range of every case of both tables (the plan's own choice at 256 CUs): an odd and an even slice count,
    both for a last range and for one that is not the last.  The ring has two stages: an odd count consumes the slice behind
    the range's end, which the descriptor's extent has to turn into zeros -- inside the image for every range but the last."""
    seen = {(n % 2, last) for c in CASES + WIDE for n, last in F.range_slices(c)}
    assert seen == {(0, False), (0, True), (1, False), (1, True)}, seen
    assert any(n == 1 and not last for c in WIDE for n, last in F.range_slices(c))
    assert {n for c in WIDE for n, _ in F.range_slices(c)} >= {1, 2, 3, 33, 43}
    # where a last range ends: in the low half of its last slice, one element into the high half, deep inside the high half
    tails = {(c.in_ - 1) % F.SLICE + 1 for c in CASES + WIDE}
    assert any(t <= F.HALF for t in tails) and F.HALF + 1 in tails and any(F.HALF + 32 <= t < F.SLICE for t in tails), tails


def test_the_reserved_workspaces_shape_has_a_plan_of_its_own():
    """tests/test_gpu_q4decode.py's reserve_decode() test: the 4-bit plan's work_bytes varies with the row count, its largest
    is not that of 16 rows, and it is not the int8 plan's -- a QWeight4 that planned through the int8 library would reserve
    another size."""
    out, in_ = F.RESERVE_SHAPE
    for cus in (256, 304, 64):
        mine = {rows: F.plan(rows, out, in_, cus=cus) for rows in range(1, F.MAX_ROWS + 1)}
        theirs = {rows: D.plan(rows, out, in_, cus=cus) for rows in range(1, F.MAX_ROWS + 1)}
        assert len({p[1] for p in mine.values()}) >= 4 and len({p[2] for p in mine.values()}) >= 3, cus
        assert max(p[1] for p in mine.values()) > mine[F.MAX_ROWS][1], cus
        assert any(mine[rows][1] != theirs[rows][1] for rows in mine), cus
    # (the issue's example: half the weight bytes, half the ranges)
    assert F.plan(16, 256, 8192, cus=256)[2] == 8 and D.plan(16, 256, 8192, cus=256)[2] == 16


def test_the_window_admits_no_pitch_whose_ring_offsets_wrap():
    """The largest pitch_n F.window_ok admits -- found by bisecting window_ok itself, not by the formula's inverse -- keeps
    the furthest slice the two-stage ring requests (F.furthest_slice) inside an `int` product and every lane's unsigned sum
    inside 32 bits, for every forced split count.  At in = 1 the margin is 5 120 bytes: one more ring stage, or 64 rows less
    in the window's formula, wraps.  tests/test_gpu_q4decode.py runs the two tightest shapes."""
    assert [F.furthest_slice(nk) for nk in (1, 2, 3, 4, 511, 512)] == [3, 3, 5, 5, 513, 513]
    for in_ in (1, 64, 65, 128, 129, 257, 384, 1153, 8192, F.MAX_RANGE_K, F.MAX_RANGE_K + 128):
        lo, hi = 4, 1 << 31                  # (window_ok(lo), not window_ok(hi)), multiples of 4
        assert F.window_ok(in_ + 3 & ~3, lo, in_) and not F.window_ok(in_ + 3 & ~3, hi, in_)
        while hi - lo > 4:
            mid = (lo + hi) // 8 * 4
            lo, hi = (mid, hi) if F.window_ok(in_ + 3 & ~3, mid, in_) else (lo, mid)
        assert lo == F.largest_pitch_n(in_), in_
        for splits in (1, 2, 3, -(-in_ // F.SLICE)):
            if D.valid_splits(in_, splits):
                for ext_w, soff, reach in F.weight_offsets(in_, lo, splits):
                    assert 0 < ext_w < soff < 1 << 31 and reach < 1 << 32, (in_, lo, splits, soff, reach)
    (ext_w, soff, reach), = F.weight_offsets(1, F.largest_pitch_n(1))
    assert (1 << 31) - soff == 5120 and soff + 64 * F.largest_pitch_n(1) >= 1 << 31 and ext_w == 63 * 11184784 + 128
    assert F.weight_offsets(129, F.largest_pitch_n(129), 1) == [(127 * 8388588 + 128, 1610608896, 2139090067)]
    assert F.weight_offsets(129, F.largest_pitch_n(129), 2) == [(63 * 8388588 + 128, 1610608896, 2139090067)] * 2


@built_lib.needs_library
def test_the_librarys_plan_says_the_same_of_every_case():
    if not built_lib.library_loads():
        pytest.skip("libmmult_hip_q4d.so (or the HIP runtime it links) is not loadable here")
    from how_to_optimize_gemm_amd import q8
    for c in CASES + WIDE:
        for out8, (pad, off) in ((False, D.Y_LAYOUTS[c.y]), (True, D.YQ_LAYOUTS[c.yq])):
            o16 = (off * (1 if out8 else 4)) % 16
            ldq = ((c.in_ + 3) & ~3) + c.x_pad
            got = q8.qlinear_decode4_plan(c.rows, c.out, c.in_, ldq=ldq, out8=out8, ldo=c.out + pad, o_mod16=o16, splits=c.splits, cu_count=256)
            assert got == F.plan(c.rows, c.out, c.in_, out8, c.out + pad, o16, c.splits, 256)[:2], c


# ---- the inputs' host-side conditions ---------------------------------------------------------------------------------------
def test_every_half_slice_moves_the_sums_of_every_case():
    """problem() and image_problem() assert their conditions themselves; here they run on the CPU for every shape the GPU module
    uses.  Library-made weights never hold -8; caller-made images hold every value in both nibble positions."""
    for c in CASES + WIDE:
        p = (F.problem if c.weight == "qweight" else F.image_problem)(c.rows, c.out, c.in_)
        assert p.acc.shape == (c.rows, c.out) and p.acc.any()
        assert (p.W.min() >= -7) == (c.weight == "qweight") or p.W.size < 64, c
    for rows, out, in_ in ((15, 273, 385), (2, 129, 129), (16, 273, 1153), (15, 273, 1153), F.PLAN_SHAPE, F.DEEP[:3],
                           (16,) + F.RESERVE_SHAPE, (16, D.FINISH_COLS + 1, 385), (3, 130, 257), (16, 257, 385), (16, 130, 129)):
        F.problem(rows, out, in_)
    for shape in ((2, 130, 1), (16, 130, 129)):   # the window's edge
        F.image_problem(*shape)
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


@pytest.mark.parametrize("in_,ranges", [(65536, 1), (131072, 2)])
def test_the_ceiling_problem_fills_the_accumulator_in_every_range(in_, ranges):
    """F.ceiling_problem asserts its conditions itself (16 x the sums reach +2^30 and -1 065 353 216 in every range of
    MAX_RANGE_K k; all but CEILING_CELLS = 4 sums stay below 2^24 and are moved by at least 90 % ... of each half slice); here
    it is made on the CPU, the forced plan is the one its GPU test runs, and the three regressions that show only near the
    sign bit are shown to change what it expects."""
    p = F.ceiling_problem(in_)
    assert p.xq.shape == (16, in_) and p.W.shape == (in_, 130) and F.CEILING_SHAPE == (16, 130) and F.CEILING_CELLS == 4
    assert (p.xq[0] == -128).all() and (p.xq[1] == 127).all() and (p.W[:, 0] == -8).all() and (p.W[:, 1] == 7).all()
    assert set(np.unique(p.W)) == set(range(-8, 8)) and set(np.unique(p.xq)) == set(range(-128, 128))
    assert int(p.acc[0, 0]) == ranges << 26 and int(p.acc[1, 0]) == ranges * -(1065353216 >> 4)
    text, _, splits, k_len = F.plan(16, 130, in_, splits=ranges)
    assert (splits, k_len) == (ranges, F.MAX_RANGE_K) and k_len // F.SLICE == 512 and "2 strips" in text
    assert F.plan(16, 130, in_ + 1, splits=ranges) == "long"
    # the kernel's side of the ceiling, restated: a logical shift, a second multiplication by 16
    part = F.partial_of_range(p.xq, p.W, 0, F.MAX_RANGE_K)
    acc16 = (16 * part.astype(np.int64)).astype(np.int32)
    assert np.array_equal(acc16 >> 4, part) and not np.array_equal((acc16.view(np.uint32) >> 4).view(np.int32), part)
    assert (part < 0).sum() > 200 and np.abs(256 * part.astype(np.int64)).max() >= 1 << 31
    # ... and each of them reaches both outputs' expected bytes: the saturated cells are not lost in the epilogue
    for out8 in (False, True):
        want = F.want_of(p, True, False, out8)
        bent = p._replace(W=np.where(np.arange(130) == 0, -7, p.W).astype(np.int8))   # channel 0 one step short of -8
        assert not np.array_equal(want[:2, 0], F.want_of(bent, True, False, out8)[:2, 0])


def test_the_large_sums_are_what_their_test_says():
    p = F.large_sums_problem()
    assert p.xq.shape == (16, 24576) and D.valid_splits(24576, 4) and D.ranges(24576, 4)[0] == 6144 <= F.MAX_RANGE_K
    assert np.abs(p.acc).max() > 1 << 24 and set(np.unique(p.W)) == {-8, 7}
