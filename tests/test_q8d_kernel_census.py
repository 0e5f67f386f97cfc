"""A census of libmmult_hip_q8d.so (tools/kernel_resources.py reads the code objects): exactly three kernels -- one partial
kernel, guarded by its descriptors and not by an EDGE twin, and the finish kernel for each output --, none with scratch or a
spill, and LDS and registers within what the plan's occupancy target assumes.  The three older libraries hold exactly the
kernels they held before this library existed (tests/golden/kernel_census_before_q8d.txt: their mangled names)."""
import os

import built_lib
import qdecode_ref as D
from built_lib import REPO

PKG = os.path.join(REPO, "how-to-optimize-gemm_amd")
Q8D_LIB = os.path.join(PKG, "libmmult_hip_q8d.so")
EXPECTED = ["qdecode_finish_kernel<false>", "qdecode_finish_kernel<true>", "qdecode_partial_kernel"]
LDS_PER_CU = 160 * 1024


def q8d_rows():
    assert os.path.exists(Q8D_LIB), "libmmult_hip_q8d.so has not been built: build_all() builds it"
    return built_lib.resources(Q8D_LIB)


def test_the_kernels_are_exactly_the_expected_symbols():
    assert sorted(r["kernel"] for r in q8d_rows()) == EXPECTED
    assert all("mmh" in r["name"] for r in q8d_rows())


def test_no_scratch_and_the_plans_occupancy_fits():
    for r in q8d_rows():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["sgpr_spill"] == 0, r
        assert r["threads"] == 256, r
        if r["kernel"] == "qdecode_partial_kernel":
            # a ring of two 16 KiB slices; the plan puts at most two workgroups on a CU (three on two) -- LDS and registers allow twice that
            assert r["lds_static"] == 2 * D.SLICE * D.STRIP, r
            assert -(-D.WG_NUM // D.WG_DEN) == 2 and LDS_PER_CU // r["lds_static"] >= 4 and built_lib.wgs(r) >= 4, r
        else:
            assert r["lds_static"] == 0 and built_lib.wgs(r) >= 8, r


def test_the_older_libraries_hold_the_kernels_they_held():
    want = {}
    for line in open(os.path.join(REPO, "tests", "golden", "kernel_census_before_q8d.txt")):
        lib, name = line.split()
        want.setdefault(lib, []).append(name)
    assert sorted(want) == ["libmmult_hip.so", "libmmult_hip_q8.so", "libmmult_hip_q8o.so"]
    for lib, names in want.items():
        got = sorted(r["name"] for r in built_lib.resources(os.path.join(PKG, lib)))
        assert got == sorted(names), (lib, sorted(set(got) ^ set(names)))
        assert not [n for n in got if "qdecode" in n]
