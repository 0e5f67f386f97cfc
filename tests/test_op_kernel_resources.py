"""The op-form instantiations (csrc/sgemm_dma5.hpp OP, csrc/launch_op.hip) in the built product library, read on the CPU
(tools/kernel_resources.py): all 36 exist, none spills, and each one's registers allow at least the workgroups per CU of
its NN twin -- the launcher takes grids and the tail split from the twins' residency, so an op kernel that needed more
registers than its twin would be launched on a grid it cannot hold."""
import built_lib
from built_lib import K2W_RING as TILES   # NL,D; ring KiB

pytestmark = built_lib.needs_library


def _twins():
    for tile, (nl_d, _) in TILES.items():
        for edge in ("false", "true"):
            for op in (1, 2, 3):
                yield (f"sgemm_mfma_dma5_op_kernel<{tile},{edge},{nl_d},{op}>", f"sgemm_mfma_dma5_kernel<{tile},{edge},{nl_d},1>", tile)
                yield (f"sgemm_dma5_op_streamk_kernel<{tile},{edge},{nl_d},{op}>", f"sgemm_dma5_streamk_kernel<{tile},{edge},true,{nl_d},1>", tile)


def test_the_36_op_instantiations_exist():
    built_lib.check_twins_exist(_twins, 36, r"sgemm_(mfma_dma5_op|dma5_op_streamk)_kernel<", "sgemm_naive_op_kernel")


def test_no_op_instantiation_spills():
    built_lib.check_no_spill([op for op, _, _ in _twins()], lambda op: 64 if "streamk" in op else 0)


def test_op_instantiations_fit_their_nn_twins_co_residency():
    built_lib.check_twins_co_residency(_twins)
