"""The batched instantiations (csrc/sgemm_dma5.hpp sgemm_mfma_dma5_batched_kernel, csrc/launch_batched.hip) in the built
product library, read on the CPU (tools/kernel_resources.py): all 24 exist with the naive batched kernel, none spills,
and each one's registers allow at least the workgroups per CU of its NN twin -- the launcher takes the tail split from
the twin's residency."""
import built_lib
from built_lib import K2W_RING as TILES   # NL,D; ring KiB

pytestmark = built_lib.needs_library


def _twins():
    for tile, (nl_d, _) in TILES.items():
        for edge in ("false", "true"):
            for op in (0, 1, 2, 3):
                yield f"sgemm_mfma_dma5_batched_kernel<{tile},{edge},{nl_d},{op}>", f"sgemm_mfma_dma5_kernel<{tile},{edge},{nl_d},1>", tile


def test_the_24_batched_instantiations_exist():
    built_lib.check_twins_exist(_twins, 24, r"sgemm_mfma_dma5_batched_kernel<", "sgemm_naive_batched_kernel")


def test_no_batched_instantiation_spills():
    built_lib.check_no_spill([b for b, _, _ in _twins()] + ["sgemm_naive_batched_kernel"])


def test_batched_instantiations_fit_their_nn_twins_co_residency():
    built_lib.check_twins_co_residency(_twins)
