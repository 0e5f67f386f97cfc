"""A census of libmmult_hip_q8.so, and the first library's symbols held still.  Every kernel in the second library's code objects
(tools/kernel_resources.py) has exactly one row in tests/test_gpu_qlinear.py::Q8_INSTANTIATIONS and every row a kernel; none
spills; the 128x128 GEMMs leave room for two workgroups per CU.  libmmult_hip.so's kernel symbols are the list recorded in
tests/golden/product_kernels.txt from the build before the int8 linear layer: the layer ships in its own library so that
nothing there is added, renamed or removed."""
import collections
import os

import built_lib
import test_kernel_census as first
from built_lib import REPO
from test_gpu_qlinear import Q8_INSTANTIATIONS

Q8_LIB = os.path.join(REPO, "how-to-optimize-gemm_amd", "libmmult_hip_q8.so")


def q8_rows():
    assert os.path.exists(Q8_LIB), "libmmult_hip_q8.so has not been built: build_all() builds it"
    return built_lib.resources(Q8_LIB)


def test_every_kernel_has_exactly_one_row_and_every_row_a_kernel():
    symbols = [first.symbol_of(r) for r in q8_rows()]
    assert len(symbols) == len(set(symbols)) == 19, symbols
    assert not any(s.startswith("_") for s in symbols), "a kernel whose template arguments kernel_resources does not print"
    rows = collections.Counter(r.symbol for r in Q8_INSTANTIATIONS)
    assert max(rows.values()) == 1, [s for s, n in rows.items() if n > 1]
    assert sorted(s for s in symbols if s not in rows) == [], "kernels of libmmult_hip_q8.so without a row"
    assert sorted(s for s in rows if s not in symbols) == [], "rows without a kernel"
    # nothing of the first library's families: the GEMM is a new shell around its tile, not a second copy of its kernels
    assert not [s for s in symbols if any(e["pattern"].search(s) for e in first.CENSUS)]


def test_no_kernel_spills_and_the_small_tile_fits_twice():
    for r in q8_rows():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["sgpr_spill"] == 0, r
        if r["kernel"].startswith("qlinear_s8_kernel<128,"):
            assert r["threads"] == 256 and built_lib.wgs(r) >= 2, r     # (LDS: 64 KiB of 160 each)
        elif r["kernel"].startswith("qlinear_s8_kernel<256,"):
            assert r["threads"] == 512 and built_lib.wgs(r) >= 1, r
        else:
            assert r["threads"] == 256 and r["vgpr"] <= 64, r            # the streaming passes: eight waves per SIMD


def test_the_first_librarys_kernel_symbols_are_the_recorded_ones():
    with open(os.path.join(REPO, "tests", "golden", "product_kernels.txt")) as f:
        recorded = f.read().split("\n")[:-1]
    assert len(recorded) == 258 and recorded == sorted(set(recorded))
    assert os.path.exists(built_lib.LIB), "libmmult_hip.so has not been built"
    assert first._symbols() == recorded
