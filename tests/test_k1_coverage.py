"""Every instantiation of the register-staged K1 kernel (sgemm_valu_kernel) in the built product library has a row in
tests/test_gpu_k1_parity.py::K1_INSTANTIATIONS, and every row names an instantiation that is there -- read on the CPU from the
library's code objects (tools/kernel_resources.py).  Every case of every row is proved here to reach its row on
csrc/launch_valu.hip's host arithmetic as that module restates it (k1_route: fast_shape for 32- and for 64-deep K-slices, the
restated window_ok, tiles >= 4 CUs with stream-K off), and the table is held to the classes it claims: the K-tail classes of
each tile's own slice depth, m and n below the tile, one, two and three or more K-slices, both operands beyond the window."""
import math
import os
import re

import pytest

import built_lib
from built_lib import REPO

pytestmark = built_lib.needs_library

FAMILY = re.compile(r"^sgemm_valu_kernel<")
CUS = 256   # the MI355X's compute units (the GPU test derives its shapes from the device's count)
ALL_CUS = (CUS, 304, 64)


def _T():
    import test_gpu_k1_parity as T
    return T


def test_the_table_names_every_k1_instantiation_of_the_library():
    rows = _T().K1_INSTANTIATIONS
    symbols = [r.symbol for r in rows]
    assert len(symbols) == len(set(symbols)), "a symbol has two rows"
    built = built_lib.built(FAMILY)
    missing = sorted(built - set(symbols))
    stale = sorted(set(symbols) - built)
    assert not missing, f"instantiations in libmmult_hip.so without a row in K1_INSTANTIATIONS: {missing}"
    assert not stale, f"rows of K1_INSTANTIATIONS that name no instantiation of libmmult_hip.so: {stale}"
    assert len(built) == 4, len(built)


def test_no_row_is_an_escape_hatch():
    """All four are reachable through mmh_sgemm with a forced valu_* id: every row runs cases, none points elsewhere."""
    for r in _T().K1_INSTANTIATIONS:
        assert not hasattr(r, "covered_by") and not hasattr(r, "unreachable"), r.symbol
        for cus in ALL_CUS:
            assert r.cases(cus), r.symbol


def test_the_rows_are_the_tiles_the_launcher_instantiates():
    """launch_valu_tile<BM, BN, KB> = launch_valu_tile_p<BM, BN, KB, 1, (BM == 64 ? 4 : 1)>, for <64,64,64> and <128,128,32>."""
    import how_to_optimize_gemm_amd as H
    T = _T()
    src = open(os.path.join(REPO, "how-to-optimize-gemm_amd", "csrc", "launch_valu.hip")).read()
    assert "return launch_valu_tile_p<BM, BN, KB, 1, (BM == 64 ? 4 : 1)>(g);" in src
    assert "return launch_valu_tile<64, 64, 64>(g);" in src and "return launch_valu_tile<128, 128, 32>(g);" in src
    for r in T.K1_INSTANTIATIONS:
        g = T.FAMILY_RE.match(r.symbol)
        assert g, r.symbol
        assert (r.bm, r.bn, r.kb) == (int(g["bm"]), int(g["bn"]), int(g["kb"])) and r.guarded == (g["edge"] == "true"), r.symbol
        assert T.K1_TILES[(r.bm, r.bn)] == (r.kb, int(g["p"])), r.symbol
        assert r.kernels and all(k in H.KERNELS for k in r.kernels), r.symbol
        assert r.kernels[0] == f"valu_{r.bm}x{r.bn}", r.symbol
        if r.guarded and r.bm == 128:
            assert set(r.kernels) == {"valu_128x128", "valu_128x64"}, r.symbol
        head = f"sgemm_valu_kernel<{r.bm},{r.bn}>"
        assert head in r.markers and ("guarded" in r.markers) == r.guarded and ("guarded" in r.absent) == (not r.guarded), r.symbol
        assert "sgemm_valu_dma5" in r.absent, r.symbol


def test_window_ok_is_the_librarys():
    """The restatement k1_route uses, against the header's text."""
    src = open(os.path.join(REPO, "how-to-optimize-gemm_amd", "csrc", "internal.hpp")).read()
    assert "const size_t lim = (1ull << 31) - 4096;" in src
    assert "return ((size_t)BM * lda + k) * 4 < lim && ((size_t)k * ldb + BN) * 4 < lim;" in src
    T = _T()
    lim = (1 << 31) - 4096
    for bm, bn, k, lda, ldb in ((64, 64, 64, 68, 68), (64, 64, 64, 68, lim // 4 // 64), (128, 128, 32, lim // 4 // 128, 132)):
        assert T.window_ok(bm, bn, k, lda, ldb) == ((bm * lda + k) * 4 < lim and (k * ldb + bn) * 4 < lim)


@pytest.mark.parametrize("cus", ALL_CUS)
def test_every_case_reaches_its_row(cus):
    T = _T()
    for r in T.K1_INSTANTIATIONS:
        for kernel in r.kernels:
            ran = 0
            for c in r.cases(cus):
                if c.kernels and kernel not in c.kernels:
                    continue
                ran += 1
                lda, ldb, ldc = r.leading_dimensions(c)
                assert lda >= c.k and ldb >= c.n and ldc >= c.n, (r.symbol, c)
                assert T.k1_route(kernel, c, (lda, ldb, ldc), cus) == ("sgemm_valu_kernel", r.bm, r.bn, r.guarded), (r.symbol, kernel, c)
                # a whole-tile shape (by the 32-deep rule K1W goes by) gets here only past the window or from four tiles per CU
                whole32 = c.aligned and c.m % r.bm == 0 and c.n % r.bn == 0 and c.k % 32 == 0
                tiles = math.ceil(c.m / r.bm) * math.ceil(c.n / r.bn)
                if whole32:
                    inside = T.window_ok(r.bm, r.bn, c.k, lda, ldb)
                    assert inside == c.production and (not c.production or (tiles >= 4 * cus and r.bm == 128)), (r.symbol, c)
                # a large operand fits the NaN buffer (run_strided: 16 bytes in, or 4)
                off = 4 if c.aligned else 1
                assert not (c.lda and c.ldb), (r.symbol, c)
                if c.lda:
                    assert off + (c.m - 1) * c.lda + c.k <= T.BIG_FLOATS, (r.symbol, c)
                if c.ldb:
                    assert off + (c.k - 1) * c.ldb + c.n <= T.BIG_FLOATS, (r.symbol, c)
                # the oracle's work per case: under 1 GFLOP; the production route's: the smallest square of four tiles per CU, two K-slices
                if c.production:
                    assert tiles < (math.isqrt(4 * cus) + 2) ** 2 and c.k == 2 * r.kb, (r.symbol, c)
                else:
                    assert 2 * c.m * c.n * c.k <= 1e9, (r.symbol, c)
            assert ran, (r.symbol, kernel)


def test_the_rows_cover_the_classes_they_claim():
    T = _T()
    for r in T.K1_INSTANTIATIONS:
        cases = r.cases(CUS)
        bm, bn, kb = r.bm, r.bn, r.kb
        nks = {math.ceil(c.k / kb) for c in cases}
        assert 1 in nks and 2 in nks and any(x >= 3 for x in nks), (r.symbol, nks)   # NBUF = 1: one slice, one parked, a steady state
        if r.guarded:
            ragged = [c for c in cases if not c.aligned]
            assert all(x % 2 == 1 for c in ragged for x in r.leading_dimensions(c)), r.symbol   # odd leading dimensions
            tails = {c.k % kb for c in ragged}
            assert {0, 1, kb - 1} <= tails, (r.symbol, tails)                                # the tile's OWN slice depth
            assert any(c.k > 2 * kb and c.k % kb for c in ragged), r.symbol                      # a tail behind two and more slices
            assert any(c.m < bm and c.n < bn for c in ragged), r.symbol                          # m and n below the tile
            assert any(c.m > bm and c.n > bn and c.m % bm and c.n % bn for c in ragged), r.symbol   # several ragged tiles
            assert any(c.m % bm == 0 and c.n % bn == 0 and c.k % kb == 0 for c in ragged), r.symbol  # guarded by alignment alone
            if kb > 32:
                # the 64-deep tile: whole by the 32-deep rule, not by its own -- `fast` with the wrong depth would take it
                trap = [c for c in cases if c.aligned]
                assert trap and all(c.m % bm == 0 and c.n % bn == 0 and c.k % 32 == 0 and c.k % kb for c in trap), r.symbol
        else:
            assert all(c.aligned and c.m % bm == 0 and c.n % bn == 0 and c.k % kb == 0 for c in cases), r.symbol
            one = [c for c in cases if (c.m, c.n, c.k) == (bm, bn, kb)]
            assert any(c.ldb for c in one) and any(c.lda for c in one), r.symbol               # B, then A, beyond the window
            for c in one:
                step = dict(lda=c.lda - 4) if c.lda else dict(ldb=c.ldb - 4)                      # the smallest that fails
                lda, ldb, _ = r.leading_dimensions(c)
                assert T.window_ok(bm, bn, c.k, step.get("lda", lda), step.get("ldb", ldb)) and not T.window_ok(bm, bn, c.k, lda, ldb)
            deep = {c.k // kb for c in cases if (c.m, c.n) == (2 * bm, 3 * bn) and c.ldb}
            assert deep == {2, 7}, (r.symbol, deep)                                              # several tiles: block_to_tile
            production = [c for c in cases if c.production]
            assert len(production) == (1 if bm == 128 else 0), r.symbol
            for c in production:
                assert c.m == c.n == 128 * math.ceil(math.sqrt(4 * CUS)) and c.k == 64 and not c.lda and not c.ldb, c


def test_the_planner_names_a_kernel_for_every_rows_shapes():
    import how_to_optimize_gemm_amd as H
    T = _T()
    for r in T.K1_INSTANTIATIONS:
        for c in r.cases(CUS):
            lda, ldb, ldc = r.leading_dimensions(c)
            name, tiles, _ = H.auto_plan(c.m, c.n, c.k, lda=lda, ldb=ldb, ldc=ldc, base_align=16 if c.aligned else 4, cu_count=CUS)
            assert name in H.KERNELS and tiles >= 1, (r.symbol, c, name, tiles)
