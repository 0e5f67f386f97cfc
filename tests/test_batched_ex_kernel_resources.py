"""The batched fused-epilogue instantiations (csrc/sgemm_dma5.hpp sgemm_mfma_dma5_batched_ex_kernel,
csrc/launch_batched_ex.hip) in the built product library, read on the CPU (tools/kernel_resources.py): all 24 exist with the
naive batched `ex` kernel, exactly 24 carry the family's name -- and none of them the batched or the `ex` family's, whose counts
other tests pin --, none spills a vector or a scalar register or uses scratch, and each one's registers allow at least the
workgroups per CU of its NN twin: the launcher takes the tail split from the twin's residency."""
import re

import built_lib
from built_lib import K2W_RING as TILES   # NL,D; ring KiB

pytestmark = built_lib.needs_library
FAMILY = r"sgemm_mfma_dma5_batched_ex_kernel<"
NAIVE = "sgemm_naive_batched_ex_kernel"


def _twins():
    for tile, (nl_d, _) in TILES.items():
        for edge in ("false", "true"):
            for op in (0, 1, 2, 3):
                yield f"sgemm_mfma_dma5_batched_ex_kernel<{tile},{edge},{nl_d},{op}>", f"sgemm_mfma_dma5_kernel<{tile},{edge},{nl_d},1>", tile


def test_the_24_batched_ex_instantiations_exist_under_a_name_of_their_own():
    rows = built_lib.check_twins_exist(_twins, 24, FAMILY, NAIVE)
    mine = [k for k in rows if re.match(FAMILY, k)]
    for k in mine + [NAIVE]:
        assert not re.match(r"^sgemm_mfma_dma5_batched_kernel<", k), k
        assert not re.match(r"^sgemm_(mfma_dma5_ex|dma5_ex_streamk)_kernel<", k), k
        assert k not in ("sgemm_naive_batched_kernel", "sgemm_naive_ex_kernel")


def test_no_batched_ex_instantiation_spills():
    built_lib.check_no_spill([b for b, _, _ in _twins()] + [NAIVE])


def test_batched_ex_instantiations_fit_their_nn_twins_co_residency():
    built_lib.check_twins_co_residency(_twins)
