"""mmh_relu_grad_colsum / mmh_time_relu_grad_colsum (include/mmult_hip.h) as far as they can be checked without a device: the
symbols, the version, the block size the header, the library's Python mirror and the contract agree on, the NULL-handle
answer, the argument checks that come before the device is touched, and the Python names."""
import ctypes as C

from built_lib import REPO


def test_the_symbols_are_exported_and_the_version_moved():
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    for s in ("mmh_relu_grad_colsum", "mmh_time_relu_grad_colsum", "mmh_kernel_has_op_forms"):
        assert hasattr(L, s), s
        assert s in H.EXPORTS, s
    assert L.mmh_version() >= 303
    assert "COLSUM_BLOCK_ROWS" in H.api.__all__


def test_the_block_rows_of_header_and_package_agree():
    import how_to_optimize_gemm_amd as H
    import relu_grad_ref as ref
    assert ref.header_block_rows(REPO) == H.COLSUM_BLOCK_ROWS
    assert H.COLSUM_BLOCK_ROWS in (64, 128, 256)


def test_a_null_handle_is_an_invalid_argument():
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert L.mmh_relu_grad_colsum(None, 2, 4, p, 4, None, 4, p, 4, None, 0, None) == H.ERR_INVALID_ARG
    ms = C.c_float()
    assert L.mmh_time_relu_grad_colsum(None, 2, 4, p, 4, None, 4, p, 4, None, 0, 1, 1, None, C.byref(ms)) == H.ERR_INVALID_ARG


def test_bad_arguments_are_refused_before_the_device_is_touched():
    """(a fake non-NULL handle is never dereferenced: the argument checks come first)"""
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    buf = (C.c_float * 64)()
    p, fake = C.cast(buf, C.c_void_p), C.c_void_p(8)
    call = lambda *a: L.mmh_relu_grad_colsum(fake, *a, None)
    assert call(2, 4, None, 4, None, 4, p, 4, p, 0) == H.ERR_INVALID_ARG     # NULL dG
    assert call(2, 4, p, 4, p, 4, None, 4, None, 0) == H.ERR_INVALID_ARG     # both outputs NULL
    assert call(2, 4, p, 3, None, 4, p, 4, p, 0) == H.ERR_INVALID_ARG        # ldg < cols
    assert call(2, 4, p, 4, p, 3, p, 4, p, 0) == H.ERR_INVALID_ARG           # ldy < cols with a gate
    assert call(2, 4, p, 4, None, 4, p, 3, p, 0) == H.ERR_INVALID_ARG        # ldz < cols with a dz
    assert call(-1, 4, p, 4, None, 4, p, 4, p, 0) == H.ERR_INVALID_ARG       # negative sizes
    assert call(2, -4, p, 4, None, 4, p, 4, p, 0) == H.ERR_INVALID_ARG
    assert all(v == 0.0 for v in buf)


def test_the_python_names_are_callable():
    import how_to_optimize_gemm_amd as H
    for name in ("relu_grad_colsum", "time_relu_grad_colsum", "linear_backward"):
        assert callable(getattr(H.MMult, name)), name
    from how_to_optimize_gemm_amd import autograd
    import torch
    assert callable(autograd.linear) and issubclass(autograd.Linear, torch.nn.Module)


def test_kernel_has_op_forms_is_the_librarys_own_answer():
    """What MMult.linear_backward asks before it launches anything: AUTO, the naive kernel and the three LDS-DMA tiles with op
    forms run mmh_sgemm_op's transposed forms and mmh_sgemm_ex; every other id of the catalogue does not."""
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    yes = {H.KERNEL_AUTO, H.KERNEL_NAIVE, H.KERNELS["mfma_64x64_dma5"], H.KERNELS["mfma_128x64_dma5"], H.KERNELS["mfma_128x128_dma5"]}
    for name, kid in H.KERNELS.items():
        assert L.mmh_kernel_has_op_forms(kid) == (1 if kid in yes else 0), name
    assert L.mmh_kernel_has_op_forms(9999) == H.ERR_INVALID_ARG
    assert L.mmh_kernel_has_op_forms(-5) == H.ERR_INVALID_ARG
