"""The case table of the int8-output layer's GPU tests (tests/test_gpu_q8o_table.py: s8o_cases) has the classes it promises,
checked on the CPU with the plan's Python restatement (tests/qchain_ref.py: plan_text_s8o) at the MI355X's 256 compute units:
every case reaches its class's instantiation with the right workgroup count; K depths of one to four trips of the tile's loop
and, for the 128 tiles, every K tail; thin last tiles in both directions for both guarded tiles; pitches of every residue
modulo 4, bases 0 - 3 bytes past a dword for the guarded rows and 0 - 12 past 16 for the whole ones; whole tiles guarded by the
base alone and by the pitch alone; ragged tiles that store dwords; a fully dense case; grids that are no multiple of the 8 XCDs,
one tile row and one tile column.  A change that drops a class from the table fails here, without a GPU.

Also here, because they need no GPU either: the host-side conditions of that module's inputs (every 128-byte slice of k moves
the expected bytes; the caller-made rows, the sums beyond 2^24 and the scale rows are what their tests say they are)."""
import math

import pytest

import built_lib
import qchain_ref as Q
import qlinear_ref as R
import test_gpu_q8o_table as T
from test_gpu_qlinear import KS_256, KS_256_EDGE, KS_Q8, THIN

CUS = 256   # the MI355X's compute units (the GPU test derives its shapes from the device's count)
CLASS_IDS = [f"{t}-{'guarded' if e else 'whole'}" for t, e in T.CLASSES]


def _last(x, tile):
    """The width of the last tile along a dimension of x."""
    return x - (math.ceil(x / tile) - 1) * tile


def _whole(c, tile):
    return c.rows % tile == 0 and c.out % tile == 0


@pytest.mark.parametrize("tile,edge", T.CLASSES, ids=CLASS_IDS)
def test_every_case_reaches_its_class(tile, edge):
    cases = T.s8o_cases(tile, edge, CUS)
    assert cases and len(set(cases)) == len(cases), (tile, edge)
    for c in cases:
        grid = math.ceil(c.rows / tile) * math.ceil(c.out / tile)
        assert Q.plan_text_s8o(c.rows, c.out, c.ldyq, c.off_y % 4, CUS) == f"{T.symbol_of(tile, edge)}, {grid} workgroups", c
        assert R.big_tile(c.rows, c.out, CUS) == (tile == 256), c
        assert c.ldyq >= c.out and c.ldq_pad in (0, 4, 8, 12) and c.off_x in (0, 4, 8, 12) and c.in_ > 0, c
    assert len(T.CLASSES) == 4 and len(set(T.CLASSES)) == 4


@pytest.mark.parametrize("tile,edge", T.CLASSES, ids=CLASS_IDS)
def test_the_classes_cover_k_depths_thin_tiles_pitches_bases_and_grids(tile, edge):
    cases = T.s8o_cases(tile, edge, CUS)
    ks = {c.in_ for c in cases}
    assert {1, 2, 3, 4} <= {math.ceil(k / 256) for k in ks}, (tile, edge, sorted(ks))   # trips of the tile's K loop
    assert {0, 4, 8, 12} <= {c.ldq_pad for c in cases} and {0, 4, 8, 12} <= {c.off_x for c in cases}, (tile, edge)
    if tile == 128:
        assert set(KS_Q8) <= ks, sorted(set(KS_Q8) - ks)
        # the last pair of slices: the odd one empty, one byte, full; tails that are no multiple of 64, 16 or 4
        assert {128, 129, 256} <= {k - 256 * (math.ceil(k / 256) - 1) for k in ks}
        assert any(k % 4 for k in ks) and any(k % 16 and not k % 4 for k in ks) and any(k % 64 and not k % 16 for k in ks)
        grids = {(math.ceil(c.rows / tile), math.ceil(c.out / tile)) for c in cases}
        assert any(a * b > 8 and (a * b) % 8 for a, b in grids), sorted(grids)
        assert any(a == 1 and b >= 17 for a, b in grids) and any(b == 1 and a >= 17 for a, b in grids), sorted(grids)
    else:
        assert set(KS_256_EDGE if edge else KS_256) <= ks, sorted(ks)
    if not edge:
        assert all(_whole(c, tile) and c.ldyq % 4 == 0 and c.off_y in (0, 4, 8, 12) for c in cases)
        assert {c.off_y for c in cases} == {0, 4, 8, 12}
        assert {c.ldyq - c.out for c in cases} >= {0, 4, 16}
        if tile == 128:   # every K depth behind a pitch above `out` and behind a base past 16; the dense case
            assert {math.ceil(c.in_ / 256) for c in cases if c.ldyq > c.out} >= {2, 3, 4}
            assert {math.ceil(c.in_ / 256) for c in cases if c.off_y} >= {2, 3, 4}
            assert any(c.ldq_pad == c.off_x == c.off_y == 0 and c.ldyq == c.out and c.in_ % 4 == 0 for c in cases), "no dense case"
        return
    for name, thin in (("rows", {_last(c.rows, tile) for c in cases if c.rows > tile}), ("out", {_last(c.out, tile) for c in cases if c.out > tile})):
        assert set(THIN) <= thin, (tile, name, sorted(set(THIN) - thin))
    ragged = [c for c in cases if not _whole(c, tile)]
    assert {c.ldyq % 4 for c in ragged} == {0, 1, 2, 3} and {c.off_y for c in cases} == {0, 1, 2, 3}, tile
    # each thin width and height meets bytes (a pitch or a base that is off) -- and the dword store, at least once per class
    assert any(c.ldyq % 4 == 0 and c.off_y == 0 and c.out % 4 for c in ragged), (tile, "no ragged tile that stores dwords")
    assert any(_whole(c, tile) and c.off_y % 4 and c.ldyq % 4 == 0 for c in cases), (tile, "not guarded by the base alone")
    assert any(_whole(c, tile) and c.off_y % 4 == 0 and c.ldyq % 2 for c in cases), (tile, "not guarded by the pitch alone")
    if tile == 128:
        assert all(S in cases for S in (T.S8oCase(c.rows, c.out, c.in_, 4, 0, c.ldyq, c.off) for c in T.C.store_cases()))
        assert any(c.rows == 1 and c.ldyq > c.out and c.out == 1 for c in cases) and any(c.rows == 1 and c.ldyq > c.out > 128 for c in cases)
        big = [c for c in cases if math.ceil(c.rows / tile) * math.ceil(c.out / tile) > 8]
        assert any(c.ldyq % 2 for c in big) and any(c.off_y for c in big)
    else:   # both misalignment cases run three trips of the K loop
        assert all(c.in_ == 513 for c in cases if _whole(c, tile))


def test_the_epilogues_of_a_class():
    assert sorted(T.EPILOGUES[128]) == [(False, False), (False, True), (True, False), (True, True)]
    assert sorted(T.EPILOGUES[256]) == [(False, True), (True, False)]


@built_lib.needs_library
def test_the_librarys_plan_says_the_same_of_every_case():
    """mmh_q8o_linear_plan (host arithmetic in libmmult_hip_q8o.so) on every case's pitches and base residues."""
    if not built_lib.library_loads():
        pytest.skip("libmmult_hip_q8o.so (or the HIP runtime it links) is not loadable here")
    from how_to_optimize_gemm_amd import q8
    for tile, edge in T.CLASSES:
        for c in T.s8o_cases(tile, edge, CUS):
            got = q8.qlinear_s8o_plan(c.rows, c.out, c.in_, T.ldq_of(c), 0, c.ldyq, c.off_x % 4, 0, c.off_y % 4, CUS)
            assert got == Q.plan_text_s8o(c.rows, c.out, c.ldyq, c.off_y % 4, CUS), (tile, edge, c)


# ---- the inputs' host-side conditions -------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", [False, True], ids=["whole", "guarded"])
def test_every_slice_of_k_moves_the_bytes_of_the_128_cases(oracle, edge):
    """deep_problem asserts its conditions itself; here it runs on the CPU for every shape of the 128 classes (the 256 classes'
    shapes take the GPU test's reference time: they are asserted there, before the launch)."""
    for shape in sorted({(c.rows, c.out, c.in_) for c in T.s8o_cases(128, edge, CUS)}):
        T.deep_problem(*shape)


def test_a_slice_that_does_not_move_the_bytes_is_noticed(oracle):
    """every_slice_moves_the_bytes bites: a problem whose second slice of x is zero fails it."""
    (w, bias, xq, rx, acc, rw, so), _ = T.deep_problem(128, 128, 257)
    dead = xq.copy()
    dead[:, 128:256] = 0
    qw, _, _ = R.quantize_rows_ref(w)
    with pytest.raises(AssertionError):
        T.every_slice_moves_the_bytes((w, bias, dead, rx, R.int_sums(dead, qw), rw, so))


def test_the_caller_made_operands_are_what_their_tests_say(oracle):
    for shape in ((37, 70, 257), (128, 128, 513)):
        T.minus128_problem(*shape)
    T.rx_problem()
    T.large_sums_problem()
    T.scale_problem()
