"""The batched fused-epilogue instantiations (csrc/sgemm_dma5.hpp sgemm_mfma_dma5_batched_ex_kernel,
csrc/launch_batched_ex.hip) in the built product library, read on the CPU (tools/kernel_resources.py): all 24 exist with the
naive batched `ex` kernel, exactly 24 carry the family's name -- and none of them the batched or the `ex` family's, whose counts
other tests pin --, none spills a vector or a scalar register or uses scratch, and each one's registers allow at least the
workgroups per CU of its NN twin: the launcher takes the tail split from the twin's residency."""
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
LIB = os.path.join(REPO, "how-to-optimize-gemm_amd", "libmmult_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libmmult_hip.so has not been built")

TILES = {"64,64,32,2,2,3": ("2,2", 48), "128,64,32,4,2,3": ("4,2", 72), "128,128,32,4,4,3": ("4,2", 96)}   # NL,D; ring KiB
FAMILY = r"sgemm_mfma_dma5_batched_ex_kernel<"
NAIVE = "sgemm_naive_batched_ex_kernel"


def _rows():
    import kernel_resources as K
    return {r["kernel"]: r for r in K.resources(LIB)}


def _wgs(r):
    alloc = (r["vgpr"] + r["agpr"] + 7) // 8 * 8
    return (4 * min(8, 512 // max(alloc, 1))) // (r["threads"] // 64)


def _twins():
    for tile, (nl_d, _) in TILES.items():
        for edge in ("false", "true"):
            for op in (0, 1, 2, 3):
                yield f"sgemm_mfma_dma5_batched_ex_kernel<{tile},{edge},{nl_d},{op}>", f"sgemm_mfma_dma5_kernel<{tile},{edge},{nl_d},1>", tile


def test_the_24_batched_ex_instantiations_exist_under_a_name_of_their_own():
    rows = _rows()
    pairs = list(_twins())
    assert len(pairs) == 24
    missing = [b for b, _, _ in pairs if b not in rows]
    assert missing == [], missing
    mine = [k for k in rows if re.match(FAMILY, k)]
    assert len(mine) == 24, len(mine)
    assert NAIVE in rows
    for k in mine + [NAIVE]:
        assert not re.match(r"^sgemm_mfma_dma5_batched_kernel<", k), k
        assert not re.match(r"^sgemm_(mfma_dma5_ex|dma5_ex_streamk)_kernel<", k), k
        assert k not in ("sgemm_naive_batched_kernel", "sgemm_naive_ex_kernel")


def test_no_batched_ex_instantiation_spills():
    rows = _rows()
    for name in [b for b, _, _ in _twins()] + [NAIVE]:
        r = rows[name]
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["sgpr_spill"] == 0, r


def test_batched_ex_instantiations_fit_their_nn_twins_co_residency():
    rows = _rows()
    for b, twin, tile in _twins():
        lds_wgs = 160 // TILES[tile][1]
        want = min(_wgs(rows[twin]), lds_wgs)
        assert min(_wgs(rows[b]), lds_wgs) >= want, (b, rows[b]["vgpr"], twin, rows[twin]["vgpr"])
