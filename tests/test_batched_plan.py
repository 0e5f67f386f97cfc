"""mmh_auto_plan_batched (include/mmult_hip.h): MMH_KERNEL_AUTO's form for a strided batch, as host arithmetic -- fold
(B shared, A and C packed: one GEMM of batch * m rows), one launch of the batched kernel on one of the three K2W tiles
that have op forms, or a loop of the per-matrix plan -- and the argument rules mmh_sgemm_batched shares.  No device."""
import ctypes as C
import os

import pytest

from built_lib import REPO, needs_loadable_library

pytestmark = needs_loadable_library()

OK, INVALID, UNSUPPORTED = 0, -1, -4
FOLD, ONE_LAUNCH, LOOP = 1, 2, 3
TILES = {29: (64, 64), 30: (128, 64), 31: (128, 128)}


def _shapes():
    out = []
    for f in ("policy_shapes_fit.txt", "policy_shapes_heldout.txt"):
        for line in open(os.path.join(REPO, "tools", f)):
            line = line.strip()
            if line and not line.startswith("#"):
                out.append(tuple(int(x) for x in line.split(",")[:3]))
    return out


def _dense(ta, tb, m, n, k):
    lda = m if ta else k
    ldb = k if tb else n
    return lda, ldb, n, (k if ta else m) * lda, (n if tb else k) * ldb, m * n


def _batched(ta, tb, m, n, k, lda, ldb, ldc, sa, sb, sc, batch, align=16):
    import how_to_optimize_gemm_amd as H
    kern, form, wgs = C.c_int(-9), C.c_int(-9), C.c_long(-9)
    rc = H.lib().mmh_auto_plan_batched(ta, tb, m, n, k, lda, ldb, ldc, sa, sb, sc, batch, align, 256, C.byref(kern),
                                       C.byref(form), C.byref(wgs))
    return rc, kern.value, form.value, wgs.value


def _op(ta, tb, m, n, k, lda, ldb, ldc, align=16):
    import how_to_optimize_gemm_amd as H
    kern, tiles, grid = C.c_int(-9), C.c_long(-9), C.c_int(-9)
    rc = H.lib().mmh_auto_plan_op(ta, tb, m, n, k, lda, ldb, ldc, align, 256, C.byref(kern), C.byref(tiles), C.byref(grid))
    return rc, kern.value, tiles.value, grid.value


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_a_batch_of_one_is_the_per_matrix_plan(ta, tb):
    for m, n, k in _shapes():
        lda, ldb, ldc, sa, sb, sc = _dense(ta, tb, m, n, k)
        rc, kern, tiles, grid = _op(ta, tb, m, n, k, lda, ldb, ldc)
        brc, bkern, form, wgs = _batched(ta, tb, m, n, k, lda, ldb, ldc, sa, sb, sc, 1)
        assert brc == rc, (m, n, k)
        if rc != OK:
            continue
        assert bkern == kern, (m, n, k, ta, tb)
        assert form in (FOLD, LOOP), (m, n, k, form)
        assert wgs == (grid if grid > 0 else tiles), (m, n, k, wgs, tiles, grid)


def test_fold_exactly_when_its_conditions_hold():
    m, n, k, batch = 256, 256, 256, 64
    lda, ldb, ldc = k, n, n
    # B shared, A and C packed, A not transposed: fold -- the NN table (N) or the op table (T) on batch * m rows
    for tb in (0, 1):
        ldb_ = k if tb else n
        rc, kern, form, wgs = _batched(0, tb, m, n, k, lda, ldb_, ldc, m * lda, 0, m * ldc, batch)
        assert rc == OK and form == FOLD, (tb, form)
        _, okern, tiles, grid = _op(0, tb, batch * m, n, k, lda, ldb_, ldc)
        assert kern == okern and wgs == (grid if grid > 0 else tiles)
    # each condition broken on its own: never fold
    broken = [
        (1, 0, m, n, m, 0, m * ldc),                    # A transposed (packed as k x m)
        (0, 0, lda, ldb, m * lda, k * ldb, m * ldc),    # packed, but B not shared
        (0, 0, lda, ldb, m * lda + 4, 0, m * ldc),      # A not packed
        (0, 0, lda, ldb, m * lda, 0, m * ldc + 4),      # C not packed
    ]
    for ta, tb, lda_, ldb_, sa, sb, sc in broken:
        rc, _, form, _ = _batched(ta, tb, m, n, k, lda_, ldb_, ldc, sa, sb, sc, batch)
        assert rc == OK and form != FOLD, (ta, sa, sb, sc)
    # batch * m above INT_MAX
    big_m, big_batch = 1 << 16, 1 << 15
    rc, _, form, _ = _batched(0, 0, big_m, 64, 64, 64, 64, 64, big_m * 64, 0, big_m * 64, big_batch)
    assert rc == OK and form != FOLD
    rc, _, form, _ = _batched(0, 0, big_m, 64, 64, 64, 64, 64, big_m * 64, 0, big_m * 64, big_batch // 2 - 1)
    assert rc == OK and form == FOLD


@pytest.mark.parametrize("batch,size", [(256, 256), (512, 128)])
def test_many_small_matrices_plan_one_launch(batch, size):
    for ta in (0, 1):
        for tb in (0, 1):
            lda, ldb, ldc, sa, sb, sc = _dense(ta, tb, size, size, size)
            rc, kern, form, wgs = _batched(ta, tb, size, size, size, lda, ldb, ldc, sa, sb, sc, batch)
            assert rc == OK and form == ONE_LAUNCH, (ta, tb, form)
            bm, bn = TILES[kern]
            assert wgs == batch * ((size + bm - 1) // bm) * ((size + bn - 1) // bn)


def test_a_few_large_matrices_loop():
    m = 2176
    lda, ldb, ldc, sa, sb, sc = _dense(0, 0, m, m, m)
    rc, kern, form, wgs = _batched(0, 0, m, m, m, lda, ldb, ldc, sa, sb, sc, 2)
    assert rc == OK and form == LOOP
    _, okern, tiles, grid = _op(0, 0, m, m, m, lda, ldb, ldc)
    assert kern == okern and wgs == 2 * (grid if grid > 0 else tiles)


def test_refusals():
    m = n = k = 64
    lda, ldb, ldc, sa, sb, sc = _dense(0, 0, m, n, k)
    assert _batched(0, 0, m, n, k, lda, ldb, ldc, sa, sb, sc, 4)[0] == OK
    assert _batched(0, 0, m, n, k, lda, ldb, ldc, sa, sb, sc, -1)[0] == INVALID
    assert _batched(0, 0, m, n, k, lda, ldb, ldc, -1, sb, sc, 4)[0] == INVALID
    assert _batched(0, 0, m, n, k, lda, ldb, ldc, sa, -1, sc, 4)[0] == INVALID
    assert _batched(0, 0, m, n, k, lda, ldb, ldc, sa, sb, -1, 4)[0] == INVALID
    bound = (m - 1) * ldc + n
    assert _batched(0, 0, m, n, k, lda, ldb, ldc, sa, sb, bound, 4)[0] == OK
    assert _batched(0, 0, m, n, k, lda, ldb, ldc, sa, sb, bound - 1, 4)[0] == INVALID
    assert _batched(0, 0, m, n, k, lda, ldb, ldc, sa, sb, 0, 4)[0] == INVALID
    assert _batched(0, 0, m, n, k, lda, ldb, ldc, sa, sb, 0, 1)[0] == OK   # (one matrix overlaps nothing)
    assert _batched(2, 0, m, n, k, lda, ldb, ldc, sa, sb, sc, 4)[0] == INVALID
    assert _batched(0, -1, m, n, k, lda, ldb, ldc, sa, sb, sc, 4)[0] == INVALID


def test_python_wrapper_names_the_form():
    import how_to_optimize_gemm_amd as H
    assert H.auto_plan_batched(0, 0, 128, 128, 128, batch=512)[1] == "one_launch"
    assert H.auto_plan_batched(0, 0, 256, 256, 256, batch=8, stride_b=0)[1] == "fold"
    assert H.auto_plan_batched(0, 0, 2176, 2176, 2176, batch=2)[1] == "loop"
