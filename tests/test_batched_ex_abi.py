"""mmh_sgemm_batched_ex / mmh_time_sgemm_batched_ex / mmh_auto_plan_batched_ex (include/mmult_hip.h) as far as they can be
checked without a device: the symbols, the version, the NULL-handle answer, the argument rules (the plan entry point runs the
call's own checks on host arithmetic alone; tests/test_gpu_batched_ex.py holds the call to them with a handle), and the plan:
the fold form only where the biases fold too, a batch of one as the per-matrix `ex` plan, many small matrices in one launch."""
import ctypes as C

import pytest

from built_lib import needs_loadable_library

pytestmark = needs_loadable_library()

NONE, COL, ROW = 0, 1, 2
FOLD, ONE_LAUNCH, LOOP = 1, 2, 3
TILE_DIMS = {29: (64, 64), 30: (128, 64), 31: (128, 128)}   # MMH_KERNEL_MFMA_{64X64,128X64,128X128}_DMA5


def _plan(ta, tb, m, n, k, lda, ldb, ldc, sa, sb, sc, sbias, mode, batch, align=16, cus=256):
    import how_to_optimize_gemm_amd as H
    kern, form, wgs = C.c_int(-9), C.c_int(-9), C.c_long(-9)
    rc = H.lib().mmh_auto_plan_batched_ex(ta, tb, m, n, k, lda, ldb, ldc, sa, sb, sc, sbias, mode, batch, align, cus, C.byref(kern),
                                          C.byref(form), C.byref(wgs))
    return rc, (kern.value, form.value, wgs.value)


def _dense(ta_, tb_, m, n, k, batch_, sbias=0, mode=NONE, **over):
    """The plan of dense packed matrices, with single arguments replaced."""
    ta, tb, batch = ta_, tb_, batch_
    lda, ldb = (m if ta else k), (k if tb else n)
    args = dict(ta=ta, tb=tb, m=m, n=n, k=k, lda=lda, ldb=ldb, ldc=n, sa=m * k, sb=k * n, sc=m * n, sbias=sbias, mode=mode, batch=batch)
    args.update(over)
    return _plan(**args)


def test_the_three_symbols_are_declared_exported_and_bound_and_the_version_moved():
    import os
    import how_to_optimize_gemm_amd as H
    from conftest import REPO
    L = H.lib()
    header = open(os.path.join(REPO, "include", "mmult_hip.h")).read()
    for s in ("mmh_sgemm_batched_ex", "mmh_time_sgemm_batched_ex", "mmh_auto_plan_batched_ex"):
        assert hasattr(L, s), s
        assert s in H.EXPORTS, s
        assert f"int {s}(" in header, s
        assert getattr(L, s).argtypes is not None, s
    assert L.mmh_version() >= 302
    for name in ("sgemm_batched_ex", "time_sgemm_batched_ex", "baddbmm", "batched_linear"):
        assert callable(getattr(H.MMult, name)), name
    assert callable(H.auto_plan_batched_ex)


def test_a_null_handle_is_an_invalid_argument():
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    assert L.mmh_sgemm_batched_ex(None, 0, 0, 4, 4, 4, 1.0, None, 4, 16, None, 4, 16, 0.0, None, 4, 16, None, 0, 0, 0, 2,
                                  None) == H.ERR_INVALID_ARG
    ms = C.c_float()
    assert L.mmh_time_sgemm_batched_ex(None, 0, 0, 4, 4, 4, 1.0, None, 4, 16, None, 4, 16, 0.0, None, 4, 16, None, 0, 0, 0, 2, 1, 1,
                                       None, C.byref(ms)) == H.ERR_INVALID_ARG


def test_argument_rules_are_settled_on_the_host():
    import how_to_optimize_gemm_amd as H
    m, n, k, batch = 300, 200, 100, 4
    ok = lambda **over: _dense(0, 0, m, n, k, batch, **over)[0]
    assert ok() == H.OK
    # operand and batch rules: mmh_sgemm_batched's
    for bad in (-1, 2, 7):
        assert ok(ta=bad) == H.ERR_INVALID_ARG and ok(tb=bad) == H.ERR_INVALID_ARG
    assert ok(sa=-1) == H.ERR_INVALID_ARG and ok(sb=-1) == H.ERR_INVALID_ARG and ok(sc=-1) == H.ERR_INVALID_ARG
    assert ok(batch=-1) == H.ERR_INVALID_ARG and ok(batch=0) == H.ERR_INVALID_ARG   # (the plan wants a batch; the call takes 0)
    assert ok(sc=(m - 1) * n + n - 1) == H.ERR_INVALID_ARG and ok(sc=(m - 1) * n + n) == H.OK   # the C-overlap rule
    assert ok(sc=0) == H.ERR_INVALID_ARG and ok(sc=0, batch=1) == H.OK
    assert ok(sa=0) == H.OK and ok(sb=0) == H.OK                                               # broadcasts
    assert ok(ldc=n - 1) == H.ERR_INVALID_ARG and ok(lda=k - 1) == H.ERR_INVALID_ARG and ok(ldb=n - 1) == H.ERR_INVALID_ARG
    assert _dense(1, 0, m, n, k, batch, lda=m - 1)[0] == H.ERR_INVALID_ARG and _dense(0, 1, m, n, k, batch, ldb=k - 1)[0] == H.ERR_INVALID_ARG
    # epilogue rules: mmh_sgemm_ex's bias modes, and the stride of the biases
    for mode in (-1, 3, 9):
        assert ok(mode=mode) == H.ERR_INVALID_ARG
    for mode in (COL, ROW):
        assert ok(mode=mode, sbias=-1) == H.ERR_INVALID_ARG
        assert ok(mode=mode, sbias=0) == H.OK and ok(mode=mode, sbias=3) == H.OK and ok(mode=mode, sbias=1 << 40) == H.OK
    assert ok(mode=NONE, sbias=-1) == H.OK   # without a bias mode the stride is ignored
    # matrices beyond the tiles' descriptor window: no `ex` kernel takes them
    assert _dense(0, 0, 1024, 1024, 1024, 2, lda=1 << 23, sa=1 << 33)[0] == H.ERR_UNSUPPORTED
    with pytest.raises(H.MMultError) as e:
        H.auto_plan_batched_ex(0, 0, m, n, k, batch=batch, bias_mode=COL, stride_bias=-1)
    assert e.value.status == H.ERR_INVALID_ARG


@pytest.mark.parametrize("tb", [0, 1])
def test_the_fold_form_needs_foldable_biases(tb):
    import how_to_optimize_gemm_amd as H
    m, n, k, batch = 128, 128, 64, 8
    fold = lambda **over: _dense(0, tb, m, n, k, batch, **{"sb": 0, **over})
    rc, one = _plan(0, tb, batch * m, n, k, k, k if tb else n, n, 0, 0, 0, 0, NONE, 1)   # the folded GEMM as a batch of one
    assert rc == H.OK
    # B shared, A and C packed: no bias, a column bias the batch shares, row biases packed m apart
    for over in (dict(), dict(mode=COL, sbias=0), dict(mode=ROW, sbias=m)):
        rc, (kern, form, wgs) = fold(**over)
        assert rc == H.OK and form == FOLD, (over, form)
        assert (kern, wgs) == (one[0], one[2]), (over, kern, wgs, one)
    name, tiles, grid = H.auto_plan_ex(0, tb, batch * m, n, k)
    assert H.kernel_name(one[0]).endswith(name) and one[2] == (grid or tiles)
    # the near misses: one launch
    for over in (dict(mode=COL, sbias=n), dict(mode=COL, sbias=1), dict(mode=ROW, sbias=0), dict(mode=ROW, sbias=m + 1),
                 dict(sb=k * n), dict(sa=m * k + 4), dict(ldc=n + 4, sc=m * (n + 4) + 4), dict(sc=m * n + 4)):
        rc, (kern, form, wgs) = fold(**over)
        assert rc == H.OK and form == ONE_LAUNCH and kern in TILE_DIMS, (over, form, kern)
    rc, (kern, form, wgs) = _dense(1, tb, m, n, k, batch, sb=0)   # transposed A is never folded
    assert rc == H.OK and form == ONE_LAUNCH
    # the Python wrapper says the same
    assert H.auto_plan_batched_ex(0, tb, m, n, k, stride_b=0, batch=batch, bias_mode=ROW, stride_bias=m)[1] == "fold"
    assert H.auto_plan_batched_ex(0, tb, m, n, k, stride_b=0, batch=batch, bias_mode=ROW, stride_bias=0)[1] == "one_launch"


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_a_batch_of_one_is_the_per_matrix_ex_plan(ta, tb):
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    for (m, n, k) in [(1024, 1024, 1024), (2176, 2176, 2176), (4096, 4096, 512), (1000, 1030, 999), (33, 17, 5), (4822, 1268, 2551)]:
        for align in (16, 4):
            for mode, sbias in ((NONE, 0), (COL, 0), (ROW, 7)):
                lda, ldb = (m if ta else k), (k if tb else n)
                rc, (kern, form, wgs) = _plan(ta, tb, m, n, k, lda, ldb, n, 0, 0, 0, sbias, mode, 1, align)
                ek, et, eg = C.c_int(), C.c_long(), C.c_int()
                assert L.mmh_auto_plan_ex(ta, tb, m, n, k, lda, ldb, n, align, 256, C.byref(ek), C.byref(et), C.byref(eg)) == H.OK
                assert rc == H.OK and form in (FOLD, LOOP), (m, n, k, form)
                assert (kern, wgs) == (ek.value, eg.value if eg.value > 0 else et.value), (m, n, k, align, mode)


def test_many_small_matrices_go_out_in_one_launch():
    import how_to_optimize_gemm_amd as H
    for ta, tb in ((0, 0), (0, 1), (1, 0), (1, 1)):
        for mode, sbias in ((NONE, 0), (COL, 64), (COL, 65), (ROW, 0)):
            rc, (kern, form, wgs) = _dense(ta, tb, 64, 64, 64, 512, sbias=sbias, mode=mode)
            assert rc == H.OK and form == ONE_LAUNCH and kern in TILE_DIMS, (ta, tb, form, kern)
            bm, bn = TILE_DIMS[kern]
            assert wgs == 512 * (-(-64 // bm)) * (-(-64 // bn))
    name, form, wgs = H.auto_plan_batched_ex(0, 1, 256, 256, 256, batch=64, bias_mode=COL, stride_bias=256)
    assert form == "one_launch" and name in ("mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5")


def test_two_large_matrices_are_a_loop_of_the_ex_plan():
    """The cube tests/test_gpu_batched_ex.py runs the loop form on is the smallest on the 128 grid, from 2176 upwards, that plans
    as one; the loop's workgroups are batch x the per-matrix `ex` plan's."""
    import how_to_optimize_gemm_amd as H
    from test_gpu_batched_ex import LOOP_CUBE
    first = next(N for N in range(2176, 8193, 128)
                 if H.auto_plan_batched_ex(0, 1, N, N, N, batch=2, bias_mode=COL, stride_bias=N + 1)[1] == "loop")
    assert first == LOOP_CUBE
    name, form, wgs = H.auto_plan_batched_ex(0, 1, first, first, first, batch=2, bias_mode=COL, stride_bias=first + 1)
    ename, tiles, grid = H.auto_plan_ex(0, 1, first, first, first)
    assert (name, wgs) == (ename, 2 * (grid or tiles))
