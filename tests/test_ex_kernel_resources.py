"""The fused-epilogue instantiations (csrc/sgemm_dma5.hpp EP, csrc/launch_ex.hip, csrc/launch_ex_t.hip) in the built product
library, read on the CPU (tools/kernel_resources.py): all 48 exist, none spills a vector register or uses scratch, the
plain ones spill no scalar register and the persistent ones at most 64, and each one's registers allow at least the
workgroups per CU of its NN twin -- the launcher takes grids, rounds and the tail split from the twins' residency
(launch_dma5.hpp), so an `ex` kernel that needed more registers than its twin would be launched on a grid it cannot hold."""
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
LIB = os.path.join(REPO, "how-to-optimize-gemm_amd", "libmmult_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libmmult_hip.so has not been built")

TILES = {"64,64,32,2,2,3": ("2,2", 48), "128,64,32,4,2,3": ("4,2", 72), "128,128,32,4,4,3": ("4,2", 96)}   # NL,D; ring KiB
# stream-K instantiations launched on their OWN residency instead of the NN twin's (a smaller persistent grid): none needed
OWN_RESIDENCY = {}


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
                yield (f"sgemm_mfma_dma5_ex_kernel<{tile},{edge},{nl_d},{op}>", f"sgemm_mfma_dma5_kernel<{tile},{edge},{nl_d},1>", tile)
                yield (f"sgemm_dma5_ex_streamk_kernel<{tile},{edge},{nl_d},{op}>", f"sgemm_dma5_streamk_kernel<{tile},{edge},true,{nl_d},1>", tile)


def test_the_48_ex_instantiations_exist():
    rows = _rows()
    pairs = list(_twins())
    assert len(pairs) == 48
    missing = [ex for ex, _, _ in pairs if ex not in rows]
    assert missing == [], missing
    n = sum(1 for k in rows if re.match(r"sgemm_(mfma_dma5_ex|dma5_ex_streamk)_kernel<", k))
    assert n == 48, n
    assert "sgemm_naive_ex_kernel" in rows


def test_no_ex_instantiation_spills():
    rows = _rows()
    for ex, _, _ in _twins():
        r = rows[ex]
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, r
        assert r["sgpr_spill"] <= (64 if "streamk" in ex else 0), r
    r = rows["sgemm_naive_ex_kernel"]
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["sgpr_spill"] == 0, r


def test_ex_instantiations_fit_their_nn_twins_co_residency():
    rows = _rows()
    for ex, twin, tile in _twins():
        lds_wgs = 160 // TILES[tile][1]
        want = min(_wgs(rows[twin]), lds_wgs)
        have = min(_wgs(rows[ex]), lds_wgs)
        if ex in OWN_RESIDENCY:
            assert "streamk" in ex and rows[ex]["vgpr"] == OWN_RESIDENCY[ex] and have >= 1, (ex, rows[ex]["vgpr"])
            continue
        assert have >= want, (ex, rows[ex]["vgpr"], twin, rows[twin]["vgpr"])
