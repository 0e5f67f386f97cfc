"""A census of libmmult_hip_q8o.so.  Every kernel in the third library's code objects (tools/kernel_resources.py) has exactly one
row in tests/test_gpu_qchain.py::Q8O_INSTANTIATIONS and every row a kernel: the four instantiations of qlinear_s8o_kernel and
nothing else; none spills or uses scratch; the 128x128 instantiations leave room for two workgroups per CU."""
import collections
import os

import built_lib
import test_kernel_census as first
from built_lib import REPO
from test_gpu_qchain import Q8O_INSTANTIATIONS

Q8O_LIB = os.path.join(REPO, "how-to-optimize-gemm_amd", "libmmult_hip_q8o.so")


def q8o_rows():
    assert os.path.exists(Q8O_LIB), "libmmult_hip_q8o.so has not been built: build_all() builds it"
    return built_lib.resources(Q8O_LIB)


def test_every_kernel_has_exactly_one_row_and_every_row_a_kernel():
    symbols = [first.symbol_of(r) for r in q8o_rows()]
    assert len(symbols) == len(set(symbols)) == 4, symbols
    assert not any(s.startswith("_") for s in symbols), "a kernel whose template arguments kernel_resources does not print"
    rows = collections.Counter(r.symbol for r in Q8O_INSTANTIATIONS)
    assert max(rows.values()) == 1, [s for s, n in rows.items() if n > 1]
    assert sorted(s for s in symbols if s not in rows) == [], "kernels of libmmult_hip_q8o.so without a row"
    assert sorted(s for s in rows if s not in symbols) == [], "rows without a kernel"
    assert sorted(rows) == sorted(f"qlinear_s8o_kernel<{t},{t},{t // 32},{e}>" for t in (128, 256) for e in ("false", "true"))
    # nothing of the first library's families, nothing of the second's: a new shell around the tile, not a copy of a kernel
    assert not [s for s in symbols if any(e["pattern"].search(s) for e in first.CENSUS)]
    assert not [s for s in symbols if s.startswith(("qlinear_s8_kernel", "quantize_rows", "prepare_weight"))]


def test_no_kernel_spills_and_the_small_tile_fits_twice():
    for r in q8o_rows():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["sgpr_spill"] == 0, r
        if r["kernel"].startswith("qlinear_s8o_kernel<128,"):
            assert r["threads"] == 256 and built_lib.wgs(r) >= 2, r     # (LDS: 64 KiB of 160 each)
        else:
            assert r["kernel"].startswith("qlinear_s8o_kernel<256,") and r["threads"] == 512 and built_lib.wgs(r) >= 1, r
