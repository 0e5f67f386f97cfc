"""A census of libmmult_hip_q4d.so (tools/kernel_resources.py reads the code objects): exactly five kernels -- the partial kernel
on packed nibbles, guarded by its descriptors and not by an EDGE twin, qdecode_s8.hpp's finish kernel for each output, and the
two kernels of the packer --, none with scratch or a spill, and LDS and registers within what the plan's occupancy target
assumes.  The int8 library's partial kernel, whose header this library reads, is NOT in it.  The four older libraries hold
exactly the kernels they held before this library existed (tests/golden/kernel_census_before_q4d.txt: their mangled names, from
a build of the commit before it)."""
import os

import built_lib
import qdecode_ref as D
from built_lib import REPO

PKG = os.path.join(REPO, "how-to-optimize-gemm_amd")
Q4D_LIB = os.path.join(PKG, "libmmult_hip_q4d.so")
EXPECTED = ["q4_pack_weight_kernel", "q4_row_amax_kernel", "q4decode_partial_kernel", "qdecode_finish_kernel<false>",
            "qdecode_finish_kernel<true>"]
LDS_PER_CU = 160 * 1024
STAGES, STAGE_BYTES = 2, 8192   # the ring shipped: two slices of [64 packed rows][128 bytes]


def q4d_rows():
    assert os.path.exists(Q4D_LIB), "libmmult_hip_q4d.so has not been built: build_all() builds it"
    return built_lib.resources(Q4D_LIB)


def test_the_kernels_are_exactly_the_expected_symbols():
    assert sorted(r["kernel"] for r in q4d_rows()) == EXPECTED
    assert all("mmh" in r["name"] for r in q4d_rows())
    assert not [r["name"] for r in q4d_rows() if "qdecode_partial_kernel" in r["name"] and "q4decode" not in r["name"]]


def test_no_scratch_and_the_plans_occupancy_fits():
    for r in q4d_rows():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["sgpr_spill"] == 0, r
        assert r["threads"] == 256, r
        if r["kernel"] == "q4decode_partial_kernel":
            assert STAGE_BYTES == D.SLICE // 2 * D.STRIP and r["lds_static"] == STAGES * STAGE_BYTES, r
            # the plan puts at most two workgroups on a CU (three on two) -- LDS and registers allow at least twice that
            assert -(-D.WG_NUM // D.WG_DEN) == 2 and LDS_PER_CU // r["lds_static"] >= 4 and built_lib.wgs(r) >= 4, r
        elif r["kernel"].startswith("qdecode_finish_kernel"):
            assert r["lds_static"] == 0 and built_lib.wgs(r) >= 8, r
        else:
            assert r["lds_static"] <= 8192, r


def test_the_finish_kernels_are_the_int8_librarys():
    """The same template of the same header: the same mangled names and the same registers as in libmmult_hip_q8d.so."""
    theirs = {r["name"]: r for r in built_lib.resources(os.path.join(PKG, "libmmult_hip_q8d.so")) if "finish" in r["name"]}
    ours = {r["name"]: r for r in q4d_rows() if "finish" in r["name"]}
    assert len(ours) == 2 and ours == theirs


def test_the_older_libraries_hold_the_kernels_they_held():
    want = {}
    for line in open(os.path.join(REPO, "tests", "golden", "kernel_census_before_q4d.txt")):
        lib, name = line.split()
        want.setdefault(lib, []).append(name)
    assert sorted(want) == ["libmmult_hip.so", "libmmult_hip_q8.so", "libmmult_hip_q8d.so", "libmmult_hip_q8o.so"]
    for lib, names in want.items():
        got = sorted(r["name"] for r in built_lib.resources(os.path.join(PKG, lib)))
        assert got == sorted(names), (lib, sorted(set(got) ^ set(names)))
        assert not [n for n in got if "q4" in n]
