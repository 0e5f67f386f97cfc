"""mmh_auto_plan_op (include/mmult_hip.h): MMH_KERNEL_AUTO's choice for transposed operands, as host arithmetic.  The op
forms run on the 64x64, 128x64 and 128x128 K2W tiles only (csrc/launch_op.hip): the plan is the fitted table restricted to
those three -- where the NN plan of a shape is one of them, the op plan is that very plan (tile, form, grid).  No device."""
import os

import pytest

from built_lib import REPO, needs_loadable_library
from built_lib import plan as _plan

pytestmark = needs_loadable_library()

OP_FAMILIES = {29, 30, 31}   # MMH_KERNEL_MFMA_{64X64,128X64,128X128}_DMA5


def _shapes():
    out = []
    for f in ("policy_shapes_fit.txt", "policy_shapes_heldout.txt"):
        for line in open(os.path.join(REPO, "tools", f)):
            line = line.strip()
            if line and not line.startswith("#"):
                out.append(tuple(int(x) for x in line.split(",")[:3]))
    return out


def test_the_three_symbols_are_exported():
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    for s in ("mmh_sgemm_op", "mmh_time_sgemm_op", "mmh_auto_plan_op"):
        assert hasattr(L, s), s
        assert s in H.EXPORTS, s
    assert (H.OP_N, H.OP_T) == (0, 1)


def test_nn_is_mmh_auto_plan_on_every_shape_of_both_sets():
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    for (m, n, k) in _shapes():
        for align in (16, 4):
            for lda, ldb, ldc in ((k, n, n), (k + 3, n + 1, n + 5)):
                a = _plan(L.mmh_auto_plan, m, n, k, lda, ldb, ldc, align, 256)
                b = _plan(L.mmh_auto_plan_op, 0, 0, m, n, k, lda, ldb, ldc, align, 256)
                assert a == b and a[0] == H.OK, (m, n, k, lda, ldb, align, a, b)


@pytest.mark.parametrize("ta,tb", [(0, 1), (1, 0), (1, 1)])
def test_op_plans_are_the_nn_plan_where_it_is_one_of_the_three_families(ta, tb):
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    same = other = 0
    for (m, n, k) in _shapes():
        for align in (16, 4):
            rc, nn = _plan(L.mmh_auto_plan, m, n, k, k, n, n, align, 256)
            assert rc == H.OK
            lda, ldb = (m if ta else k), (k if tb else n)
            rc, op = _plan(L.mmh_auto_plan_op, ta, tb, m, n, k, lda, ldb, n, align, 256)
            assert rc == H.OK, (m, n, k, rc)
            assert op[0] in OP_FAMILIES, (m, n, k, op)
            if nn[0] in OP_FAMILIES:
                assert op == nn, (m, n, k, ta, tb, align, nn, op)
                same += 1
            else:
                other += 1
    assert same > 100 and other > 10, (same, other)


def test_argument_checks_follow_the_stored_layouts():
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    m, n, k = 300, 200, 100
    ok = lambda *a: _plan(L.mmh_auto_plan_op, *a)[0]
    assert ok(0, 0, m, n, k, k, n, n, 16, 256) == H.OK
    assert ok(1, 0, m, n, k, m, n, n, 16, 256) == H.OK
    assert ok(1, 0, m, n, k, k, n, n, 16, 256) == H.ERR_INVALID_ARG      # op T: lda >= m, even though lda >= k
    assert ok(0, 0, m, n, k, m - 250, n, n, 16, 256) == H.ERR_INVALID_ARG   # op N: lda >= k
    assert ok(0, 1, m, n, k, k, k, n, 16, 256) == H.OK
    assert ok(0, 1, m, n, k, k, n, n, 16, 256) == H.OK                   # ldb = 200 >= k
    assert ok(0, 1, m, n, 250, 250, 249, n, 16, 256) == H.ERR_INVALID_ARG  # op T: ldb >= k, even though ldb >= n
    assert ok(0, 0, m, n, 250, 250, 199, n, 16, 256) == H.ERR_INVALID_ARG  # op N: ldb >= n
    assert ok(1, 1, m, n, k, m, k, n - 1, 16, 256) == H.ERR_INVALID_ARG  # ldc >= n always
    for bad in (-1, 2, 7):
        assert ok(bad, 0, m, n, k, k, n, n, 16, 256) == H.ERR_INVALID_ARG
        assert ok(0, bad, m, n, k, k, n, n, 16, 256) == H.ERR_INVALID_ARG
    for dims in ((0, n, k), (m, 0, k), (m, n, 0)):
        assert ok(1, 1, *dims, max(dims[0], 1), max(dims[2], 1), n, 16, 256) == H.ERR_INVALID_ARG


def test_operands_beyond_the_descriptor_window_are_unsupported_for_op_forms():
    """A huge lda: the NN plan falls back to a register-staged tile (no descriptor window there); the op forms have no such
    fallback and say so."""
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    m, n, k, lda = 1024, 1024, 1024, 1 << 23
    rc, nn = _plan(L.mmh_auto_plan, m, n, k, lda, n, n, 16, 256)
    assert rc == H.OK and nn[0] not in OP_FAMILIES | {7, 26, 100}, nn
    for ta, tb in ((1, 0), (1, 1), (0, 1)):
        ld_a = lda if ta else k
        ld_b = n if not tb else k
        if not ta:
            ld_b = lda                                                        # NT: the huge stride on B^T
        rc, _ = _plan(L.mmh_auto_plan_op, ta, tb, m, n, k, ld_a, ld_b, n, 16, 256)
        assert rc == H.ERR_UNSUPPORTED, (ta, tb, rc)
    # ... while the same op forms with dense operands plan normally
    for ta, tb in ((1, 0), (1, 1), (0, 1)):
        rc, op = _plan(L.mmh_auto_plan_op, ta, tb, m, n, k, m if ta else k, k if tb else n, n, 16, 256)
        assert rc == H.OK and op[0] in OP_FAMILIES


def test_python_auto_plan_op_names_the_tile():
    import how_to_optimize_gemm_amd as H
    assert H.auto_plan_op(H.OP_N, H.OP_N, 4096, 4096, 4096) == H.auto_plan(4096, 4096, 4096)
    for ta, tb in ((0, 1), (1, 0), (1, 1)):
        name, tiles, grid = H.auto_plan_op(ta, tb, 4096, 4096, 4096)
        assert name in ("mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5"), name
