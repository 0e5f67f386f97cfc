"""mmh_sgemm_ex / mmh_time_sgemm_ex / mmh_auto_plan_ex (include/mmult_hip.h): the fused-epilogue entry points as far as they
can be checked without a device -- the symbols, the NULL-handle answer, and the plan: an epilogue call is planned like an op
form (the fitted table restricted to the 64x64, 128x64 and 128x128 K2W tiles, the only ones with `ex` kernels) for NN too,
and where mmh_sgemm's own plan is one of the three it is that very plan -- the epilogue is not priced."""
import ctypes as C

import pytest

from built_lib import needs_loadable_library
from built_lib import plan as _plan

pytestmark = needs_loadable_library()

EX_FAMILIES = {29, 30, 31}   # MMH_KERNEL_MFMA_{64X64,128X64,128X128}_DMA5
SWEEP = [(n, n, n) for n in range(1024, 4097, 128)]   # the reference sweep
RAGGED = [(1000, 1030, 999), (1025, 1025, 1025), (33, 17, 5), (1, 1, 1), (7, 300, 1), (4096, 4096, 512), (2304, 2176, 320),
          (4822, 1268, 2551), (100, 5000, 64)]


def test_the_three_symbols_are_exported_and_the_version_moved():
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    for s in ("mmh_sgemm_ex", "mmh_time_sgemm_ex", "mmh_auto_plan_ex"):
        assert hasattr(L, s), s
        assert s in H.EXPORTS, s
    assert L.mmh_version() >= 301
    assert (H.BIAS_NONE, H.BIAS_COL, H.BIAS_ROW) == (0, 1, 2) and (H.ACT_NONE, H.ACT_RELU) == (0, 1)
    for name in ("sgemm_ex", "time_sgemm_ex", "addmm", "linear"):
        assert callable(getattr(H.MMult, name)), name


def test_a_null_handle_is_an_invalid_argument():
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    assert L.mmh_sgemm_ex(None, 0, 0, 4, 4, 4, 1.0, None, 4, None, 4, 0.0, None, 4, None, 0, 0, None) == H.ERR_INVALID_ARG
    ms = C.c_float()
    assert L.mmh_time_sgemm_ex(None, 0, 0, 4, 4, 4, 1.0, None, 4, None, 4, 0.0, None, 4, None, 0, 0, 1, 1, None,
                               C.byref(ms)) == H.ERR_INVALID_ARG


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_ex_plans_are_one_of_the_three_tiles_and_the_op_plan(ta, tb):
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    same_as_nn = 0
    for (m, n, k) in SWEEP + RAGGED:
        for align in (16, 4):
            lda, ldb = (m if ta else k), (k if tb else n)
            rc, ex = _plan(L.mmh_auto_plan_ex, ta, tb, m, n, k, lda, ldb, n, align, 256)
            assert rc == H.OK, (m, n, k, rc)
            assert ex[0] in EX_FAMILIES, (m, n, k, ex)
            assert ex[1] > 0 and ex[2] >= 0, ex
            if ta or tb:
                rc, op = _plan(L.mmh_auto_plan_op, ta, tb, m, n, k, lda, ldb, n, align, 256)
                assert rc == H.OK and ex == op, (m, n, k, ta, tb, align, ex, op)
            rc, nn = _plan(L.mmh_auto_plan, m, n, k, k, n, n, align, 256)
            assert rc == H.OK
            if nn[0] in EX_FAMILIES:
                assert ex == nn, (m, n, k, ta, tb, align, nn, ex)
                same_as_nn += 1
    assert same_as_nn > 20, same_as_nn


def test_the_nn_ex_plan_is_the_nt_op_plan_with_dense_operands():
    """An NN epilogue call sees the table an op form sees: with square dense operands of the same alignment its plan is the NT one."""
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    for (m, n, k) in SWEEP:
        assert _plan(L.mmh_auto_plan_ex, 0, 0, m, n, k, k, n, n, 16, 256) == _plan(L.mmh_auto_plan_op, 0, 1, m, n, k, k, k, n, 16, 256)


def test_bad_op_flags_and_shapes_are_refused():
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    m, n, k = 300, 200, 100
    ok = lambda *a: _plan(L.mmh_auto_plan_ex, *a)[0]
    assert ok(0, 0, m, n, k, k, n, n, 16, 256) == H.OK
    for bad in (-1, 2, 7):
        assert ok(bad, 0, m, n, k, k, n, n, 16, 256) == H.ERR_INVALID_ARG
        assert ok(0, bad, m, n, k, k, n, n, 16, 256) == H.ERR_INVALID_ARG
    assert ok(1, 0, m, n, k, k, n, n, 16, 256) == H.ERR_INVALID_ARG       # op T: lda >= m
    assert ok(0, 1, m, n, 250, 250, 249, n, 16, 256) == H.ERR_INVALID_ARG   # op T: ldb >= k
    assert ok(0, 0, m, n, k, k, n, n - 1, 16, 256) == H.ERR_INVALID_ARG   # ldc >= n
    # operands beyond the tiles' descriptor window: NN too has no `ex` kernel to fall back to
    assert ok(0, 0, 1024, 1024, 1024, 1 << 23, 1024, 1024, 16, 256) == H.ERR_UNSUPPORTED
    with pytest.raises(H.MMultError):
        H.auto_plan_ex(2, 0, m, n, k)


def test_python_auto_plan_ex_names_the_tile():
    import how_to_optimize_gemm_amd as H
    for ta, tb in ((0, 0), (0, 1), (1, 0), (1, 1)):
        name, tiles, grid = H.auto_plan_ex(ta, tb, 4096, 4096, 4096)
        assert name in ("mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5"), name
        assert tiles > 0
