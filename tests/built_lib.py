"""The built product library, read on the CPU: where it is, the marker that skips a module while it has not been built, its
kernels' resources (tools/kernel_resources.py reads them from the code objects embedded in the .so), and the checks every
"instantiations and their NN twins" module runs on them.  (Shared test code: see tests/bitcmp.py.)"""
import ctypes as C
import functools
import os
import re
import struct
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "how-to-optimize-gemm_amd", "libmmult_hip.so")
if os.path.join(REPO, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(REPO, "tools"))    # the one place that puts tools/ on the path

needs_library = pytest.mark.skipif(not os.path.exists(LIB), reason="libmmult_hip.so has not been built")

# the K2W tiles that have op, `ex` and batched forms: template arguments -> (NL,D; the ring's KiB of LDS)
K2W_RING = {"64,64,32,2,2,3": ("2,2", 48), "128,64,32,4,2,3": ("4,2", 72), "128,128,32,4,4,3": ("4,2", 96)}


def resources(lib=LIB):
    import kernel_resources as K
    return K.resources(lib)


def rows():
    """kernel name -> its resources"""
    return {r["kernel"]: r for r in resources()}


def built(family):
    """The kernels of the library whose name the compiled pattern `family` matches."""
    return {r["kernel"] for r in resources() if family.match(r["kernel"])}


def wgs(r):
    """Workgroups per CU the kernel's registers allow."""
    alloc = (r["vgpr"] + r["agpr"] + 7) // 8 * 8
    return (4 * min(8, 512 // max(alloc, 1))) // (r["threads"] // 64)


@functools.lru_cache(maxsize=None)
def library_loads():
    """The planners are host arithmetic, but they live in libmmult_hip.so (a hipcc build that needs the HIP runtime to LOAD):
    on a machine without the library or without libamdhip64 their tests skip, not error."""
    try:
        import how_to_optimize_gemm_amd as H
        H.lib()
        return True
    except Exception:
        return False


def needs_loadable_library():
    return pytest.mark.skipif(not library_loads(), reason="libmmult_hip.so (or the HIP runtime it links) is not loadable here")


def plan(fn, *args):
    """(status, (kernel id, tiles, grid)) of one of the library's mmh_auto_plan* entry points."""
    kern, tiles, grid = C.c_int(-9), C.c_long(-9), C.c_int(-9)
    rc = fn(*args, C.byref(kern), C.byref(tiles), C.byref(grid))
    return rc, (kern.value, tiles.value, grid.value)


def dynamic_exports(path):
    """Names of the defined global functions in an ELF64 shared object's dynamic symbol table."""
    blob = open(path, "rb").read()
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    names = []
    for _, sh_type, _, _, off, size, link, _, _, entsize in sections:
        if sh_type != 11:   # SHT_DYNSYM
            continue
        stroff = sections[link][4]
        for p in range(off, off + size, entsize):
            st_name, st_info, _, st_shndx = struct.unpack_from("<IBBH", blob, p)
            if st_shndx != 0 and (st_info & 15) == 2 and (st_info >> 4) in (1, 2):   # defined, FUNC, GLOBAL / WEAK
                names.append(blob[stroff + st_name:blob.index(b"\0", stroff + st_name)].decode())
    return sorted(names)


# ---- instantiations and their NN twins: twins() yields (instantiation, NN twin, tile) ----------------------------------------
def check_twins_exist(twins, count, family, naive):
    """All `count` instantiations are in the library, exactly `count` kernels carry the family's name (a regular expression),
    and the naive kernel is there.  Returns the resource rows."""
    have = rows()
    pairs = list(twins())
    assert len(pairs) == count, (len(pairs), count)
    missing = [x for x, _, _ in pairs if x not in have]
    assert missing == [], missing
    n = sum(1 for k in have if re.match(family, k))
    assert n == count, (family, n)
    assert naive in have, naive
    return have


def check_no_spill(names, sgpr_spills=lambda name: 0):
    """No vector spill, no scratch, and at most sgpr_spills(name) scalar spills in every kernel of `names`."""
    have = rows()
    for name in names:
        r = have[name]
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, r
        assert r["sgpr_spill"] <= sgpr_spills(name), r


def check_twins_co_residency(twins, own_residency=None):
    """Each instantiation's registers allow at least the workgroups per CU of its NN twin (the LDS ring caps both)."""
    have = rows()
    for x, twin, tile in twins():
        lds_wgs = 160 // K2W_RING[tile][1]
        want = min(wgs(have[twin]), lds_wgs)
        got = min(wgs(have[x]), lds_wgs)
        if own_residency and x in own_residency:
            assert "streamk" in x and have[x]["vgpr"] == own_residency[x] and got >= 1, (x, have[x]["vgpr"])
            continue
        assert got >= want, (x, have[x]["vgpr"], twin, have[twin]["vgpr"])
