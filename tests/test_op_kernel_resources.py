"""The op-form instantiations (csrc/sgemm_dma5.hpp OP, csrc/launch_op.hip) in the built product library, read on the CPU
(tools/kernel_resources.py): all 36 exist, none spills, and each one's registers allow at least the workgroups per CU of
its NN twin -- the launcher takes grids and the tail split from the twins' residency, so an op kernel that needed more
registers than its twin would be launched on a grid it cannot hold."""
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
LIB = os.path.join(REPO, "how-to-optimize-gemm_amd", "libmmult_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libmmult_hip.so has not been built")

TILES = {"64,64,32,2,2,3": ("2,2", 48), "128,64,32,4,2,3": ("4,2", 72), "128,128,32,4,4,3": ("4,2", 96)}   # NL,D; ring KiB


def _rows():
    import kernel_resources as K
    return {r["kernel"]: r for r in K.resources(LIB)}


def _wgs(r):
    alloc = (r["vgpr"] + r["agpr"] + 7) // 8 * 8
    return (4 * min(8, 512 // max(alloc, 1))) // (r["threads"] // 64)


def _twins():
    for tile, (nl_d, _) in TILES.items():
        for edge in ("false", "true"):
            for op in (1, 2, 3):
                yield (f"sgemm_mfma_dma5_op_kernel<{tile},{edge},{nl_d},{op}>", f"sgemm_mfma_dma5_kernel<{tile},{edge},{nl_d},1>", tile)
                yield (f"sgemm_dma5_op_streamk_kernel<{tile},{edge},{nl_d},{op}>", f"sgemm_dma5_streamk_kernel<{tile},{edge},true,{nl_d},1>", tile)


def test_the_36_op_instantiations_exist():
    rows = _rows()
    pairs = list(_twins())
    assert len(pairs) == 36
    missing = [op for op, _, _ in pairs if op not in rows]
    assert missing == [], missing
    n = sum(1 for k in rows if re.match(r"sgemm_(mfma_dma5_op|dma5_op_streamk)_kernel<", k))
    assert n == 36, n
    assert "sgemm_naive_op_kernel" in rows


def test_no_op_instantiation_spills():
    rows = _rows()
    for op, _, _ in _twins():
        r = rows[op]
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, r
        assert r["sgpr_spill"] <= (64 if "streamk" in op else 0), r


def test_op_instantiations_fit_their_nn_twins_co_residency():
    rows = _rows()
    for op, twin, tile in _twins():
        lds_wgs = 160 // TILES[tile][1]
        want = min(_wgs(rows[twin]), lds_wgs)
        assert min(_wgs(rows[op]), lds_wgs) >= want, (op, rows[op]["vgpr"], twin, rows[twin]["vgpr"])
