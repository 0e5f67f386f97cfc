"""A census of libmmult_hip_q4g.so (tools/kernel_resources.py reads the code objects): exactly four kernels -- the partial kernel
with one scale per slice, its own finish kernel for each output, and the one kernel of the packer --, none with scratch or a
spill, and LDS and registers within what the plan's occupancy target assumes.  The partial kernels of the int8 and of the
per-channel 4-bit library, whose headers this library reads, are NOT in it.  The five older libraries hold exactly the kernels
they held before this library existed (tests/golden/kernel_census_before_q4g.txt: their mangled names, from a build of the
commit before it)."""
import os

import built_lib
import qdecode_ref as D
from built_lib import REPO

PKG = os.path.join(REPO, "how-to-optimize-gemm_amd")
Q4G_LIB = os.path.join(PKG, "libmmult_hip_q4g.so")
EXPECTED = ["q4g_pack_weight_kernel", "q4gdecode_finish_kernel<false>", "q4gdecode_finish_kernel<true>", "q4gdecode_partial_kernel"]
LDS_PER_CU = 160 * 1024
STAGES, STAGE_BYTES = 2, 8192   # the ring: two slices of [64 packed rows][128 bytes], as the per-channel kernel's


def q4g_rows():
    assert os.path.exists(Q4G_LIB), "libmmult_hip_q4g.so has not been built: build_all() builds it"
    return built_lib.resources(Q4G_LIB)


def test_the_kernels_are_exactly_the_expected_symbols():
    assert sorted(r["kernel"] for r in q4g_rows()) == EXPECTED
    assert all("mmh" in r["name"] for r in q4g_rows())
    # nothing of the libraries whose headers it reads: no qdecode_partial_kernel, no q4decode_partial_kernel, none of their
    # finish or packer kernels -- every kernel here carries this library's own name
    assert all("q4gdecode_" in r["kernel"] or "q4g_pack_" in r["kernel"] for r in q4g_rows())
    assert not [r["name"] for r in q4g_rows() if "q4decode_partial" in r["name"] or "22qdecode_partial" in r["name"] or "_in_q8d_only" in r["name"]]


def test_no_scratch_and_the_plans_occupancy_fits():
    for r in q4g_rows():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["sgpr_spill"] == 0, r
        assert r["threads"] == 256, r
        if r["kernel"] == "q4gdecode_partial_kernel":
            assert STAGE_BYTES == D.SLICE // 2 * D.STRIP and r["lds_static"] == STAGES * STAGE_BYTES, r
            # the plan puts at most two workgroups on a CU (three on two) -- LDS and registers allow at least twice that
            assert -(-D.WG_NUM // D.WG_DEN) == 2 and LDS_PER_CU // r["lds_static"] >= 4 and built_lib.wgs(r) >= 4, r
        elif r["kernel"].startswith("q4gdecode_finish_kernel"):
            assert r["lds_static"] == 0 and built_lib.wgs(r) >= 8, r
        else:
            assert r["lds_static"] <= 8192, r


def test_the_older_libraries_hold_the_kernels_they_held():
    want = {}
    for line in open(os.path.join(REPO, "tests", "golden", "kernel_census_before_q4g.txt")):
        lib, name = line.split()
        want.setdefault(lib, []).append(name)
    assert sorted(want) == ["libmmult_hip.so", "libmmult_hip_q4d.so", "libmmult_hip_q8.so", "libmmult_hip_q8d.so", "libmmult_hip_q8o.so"]
    for lib, names in want.items():
        got = sorted(r["name"] for r in built_lib.resources(os.path.join(PKG, lib)))
        assert got == sorted(names), (lib, sorted(set(got) ^ set(names)))
        assert not [n for n in got if "q4g" in n]
