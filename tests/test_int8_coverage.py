"""Every int8 GEMM and quantiser instantiation in the built product library has a row in the exact-reference table
(tests/test_gpu_int8_parity.py::INSTANTIATIONS), and every row names an instantiation that is there -- read on the CPU from
the library's code objects (tools/kernel_resources.py).  Every case of every row is also checked here, on the launchers'
host arithmetic restated in tests/int8_ops.py (whole tiles, the tile rule at 256 CUs, the in-place test, quant_vec_ok and
K3p's grid): it must reach its row's instantiation, and the table must cover the classes the rows promise."""
import math
import re

import pytest

import built_lib
import int8_ops

pytestmark = built_lib.needs_library

FAMILY = re.compile(r"^(igemm_s8_simple_kernel|igemm_s8_dma_kernel|igemm_s8_pp_kernel)<|^(absmax_kernel|quantize_kernel|"
                    r"dequantize_kernel)$")
CUS = 256   # the MI355X's compute units (the GPU test derives its shapes from the device's count)


def _table():
    import test_gpu_int8_parity as T
    return T


def test_the_table_names_every_int8_instantiation_of_the_library():
    T = _table()
    symbols = [r.symbol for r in T.INSTANTIATIONS]
    assert len(symbols) == len(set(symbols)), "a symbol has two rows"
    built = built_lib.built(FAMILY)
    missing = sorted(built - set(symbols))
    stale = sorted(set(symbols) - built)
    assert not missing, f"int8 instantiations in libmmult_hip.so without a row in INSTANTIATIONS: {missing}"
    assert not stale, f"rows of INSTANTIATIONS that name no instantiation of libmmult_hip.so: {stale}"
    assert len(built) == 15, len(built)


@pytest.mark.parametrize("row", range(15))
def test_every_case_reaches_its_row(row):
    T = _table()
    inst = T.INSTANTIATIONS[row]
    cases = inst.cases(CUS)
    assert cases, inst.symbol
    for c in cases:
        entry = c.entry or inst.entry
        mode = inst.mode if c.mode is None else c.mode
        syms, _ = int8_ops.reach(entry, mode, c, CUS)
        assert inst.symbol in syms, (inst.symbol, c, syms)
    if inst.worst:
        c = inst.worst(CUS)
        assert inst.entry == "igemm" and int8_ops.reach("igemm", c.mode, c, CUS)[0] == [inst.symbol], (inst.symbol, c)
        assert 16384 * c.k <= int8_ops.INT32_MAX and 16384 * (c.k + 64) > int8_ops.INT32_MAX, c.k   # the deepest k the kernel takes
    if inst.persistent:
        for c in T._persistent_cases(inst, CUS):
            syms, words = int8_ops.reach(inst.entry, inst.mode, c, CUS, env_cap=T.GRID_CAP)
            assert inst.symbol in syms and any(w.startswith("persistent") for w in words), (inst.symbol, c, words)


def test_the_gemm_rows_cover_thin_tiles_k_tails_layouts_and_c_windows():
    T = _table()
    for inst in T.INSTANTIATIONS:
        if inst.entry != "igemm":
            continue
        cases = inst.cases(CUS)
        tile = 256 if "pp_kernel" in inst.symbol or "<256," in inst.symbol else 128
        edge = "<true" in inst.symbol or ",true,0" in inst.symbol
        ks = {c.k for c in cases}
        if "simple_kernel<false>" in inst.symbol:
            assert all(k % 64 == 0 for k in ks)
        else:
            assert set(T.KS) <= ks, (inst.symbol, sorted(set(T.KS) - ks))
        assert any(c.lda and c.lda % 4 == 0 and c.lda > c.k for c in cases), inst.symbol   # padded leading dimensions
        if edge:
            thin = {x - (math.ceil(x / tile) - 1) * tile for c in cases for x in (c.m, c.n) if x > tile}
            assert set(T.THIN) <= thin, (inst.symbol, sorted(set(T.THIN) - thin))
            lds = {(c.ldc - c.n) for c in cases if c.ldc}
            assert {1, 3} <= lds and any(c.oc == 1 for c in cases), inst.symbol
            assert any(c.m % tile == 0 and c.n % tile == 0 for c in cases), inst.symbol   # EDGE on whole tiles
        if inst.symbol in ("igemm_s8_simple_kernel<true>", "igemm_s8_dma_kernel<128,128,4,true,0,true>"):
            offs = {c.oa % 4 for c in cases} | {c.ob % 4 for c in cases}
            assert {1, 2, 3} <= offs and any(c.lda % 2 for c in cases if c.lda), inst.symbol


def test_the_quantiser_rows_cover_both_paths_and_the_lopsided_pairs():
    T = _table()
    by = {i.symbol: i for i in T.INSTANTIATIONS}
    quant = [c for c in by["absmax_kernel"].cases(CUS)]
    words = set()
    for c in quant:
        words |= set(int8_ops.reach("quantize", 0, c, CUS)[1])
    assert {"absmax_kernel (vector path)", "absmax_kernel (row path)", "quantize_kernel (vector path)",
            "quantize_kernel (row path)"} <= words
    assert {1, 2, 3, 4, 5, 4097} <= {c.n for c in quant}
    vec_thin = [c for c in quant if c.n < 4 and int8_ops.quant_vec_ok(c.lds("quantize")[0], 4 * c.oa) and c.m > 1]
    assert vec_thin, "no 1 - 3 column tensor on the vector path"
    wg = [math.ceil(c.m * max(1, math.ceil((c.n // 4) / 1024)) / 4) for c in quant
          if int8_ops.quant_vec_ok(c.lds("quantize")[0], 4 * c.oa)]
    assert max(wg) > 64, "no vector-path tensor spreads over more than AMAX_WORDS workgroups"
    values = by["quantize_kernel"].cases(CUS)
    assert any(c.values == "ties" for c in values)
    q = [c for c in values if c.entry == "qgemm"]
    assert any(c.m * c.k >= 64 * c.k * c.n for c in q) and any(c.k * c.n >= 64 * c.m * c.k for c in q)   # lopsided pairs
    two_pass = by["dequantize_kernel"].cases(CUS)
    assert any(c.oc and c.ldc > c.n for c in two_pass) and any(c.oa or c.ob for c in two_pass)
