"""The fused-epilogue instantiations (csrc/sgemm_dma5.hpp EP, csrc/launch_ex.hip, csrc/launch_ex_t.hip) in the built product
library, read on the CPU (tools/kernel_resources.py): all 48 exist, none spills a vector register or uses scratch, the
plain ones spill no scalar register and the persistent ones at most 64, and each one's registers allow at least the
workgroups per CU of its NN twin -- the launcher takes grids, rounds and the tail split from the twins' residency
(launch_dma5.hpp), so an `ex` kernel that needed more registers than its twin would be launched on a grid it cannot hold."""
import built_lib
from built_lib import K2W_RING as TILES   # NL,D; ring KiB

pytestmark = built_lib.needs_library
# stream-K instantiations launched on their OWN residency instead of the NN twin's (a smaller persistent grid): none needed
OWN_RESIDENCY = {}


def _twins():
    for tile, (nl_d, _) in TILES.items():
        for edge in ("false", "true"):
            for op in (0, 1, 2, 3):
                yield (f"sgemm_mfma_dma5_ex_kernel<{tile},{edge},{nl_d},{op}>", f"sgemm_mfma_dma5_kernel<{tile},{edge},{nl_d},1>", tile)
                yield (f"sgemm_dma5_ex_streamk_kernel<{tile},{edge},{nl_d},{op}>", f"sgemm_dma5_streamk_kernel<{tile},{edge},true,{nl_d},1>", tile)


def test_the_48_ex_instantiations_exist():
    built_lib.check_twins_exist(_twins, 48, r"sgemm_(mfma_dma5_ex|dma5_ex_streamk)_kernel<", "sgemm_naive_ex_kernel")


def test_no_ex_instantiation_spills():
    built_lib.check_no_spill([ex for ex, _, _ in _twins()] + ["sgemm_naive_ex_kernel"], lambda ex: 64 if "streamk" in ex else 0)


def test_ex_instantiations_fit_their_nn_twins_co_residency():
    built_lib.check_twins_co_residency(_twins, OWN_RESIDENCY)
