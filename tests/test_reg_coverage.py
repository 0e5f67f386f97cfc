"""Every register-staged MFMA instantiation in the built product library has a row in the oracle parity table
(tests/test_gpu_reg_parity.py::REG_INSTANTIATIONS), and every row names an instantiation that is there -- read on the CPU from
the library's code objects (tools/kernel_resources.py).  An instantiation that ships without a row fails here, by name, before
anything runs on a GPU.  The rows' shapes are checked here too, on the host arithmetic the launchers use: that each one
reaches its row's instantiation (whole or guarded for the tile's K-slice depth, ragged or whole-round tile counts, inside or
beyond the descriptor window), and the Python restatement of window_ok against the library's own (mmh_auto_plan)."""
import math
import os
import re

import built_lib
from built_lib import REPO

pytestmark = built_lib.needs_library

FAMILIES = ("sgemm_mfma_kernel", "sgemm_mfma_streamk_kernel", "sgemm_mfma_simple_kernel")   # (split-K: tests/test_splitk_coverage.py)
FAMILY = re.compile(r"^(" + "|".join(FAMILIES) + r")<")
CUS = 256   # the MI355X's compute units (the GPU test derives its shapes from the device's count)


def _T():
    import test_gpu_reg_parity as T
    return T


def test_the_table_names_every_register_staged_instantiation_of_the_library():
    rows = _T().REG_INSTANTIATIONS
    symbols = [r.symbol for r in rows]
    assert len(symbols) == len(set(symbols)), "a symbol has two rows"
    built = built_lib.built(FAMILY)
    missing = sorted(built - set(symbols))
    stale = sorted(set(symbols) - built)
    assert not missing, f"instantiations in libmmult_hip.so without a row in REG_INSTANTIATIONS: {missing}"
    assert not stale, f"rows of REG_INSTANTIATIONS that name no instantiation of libmmult_hip.so: {stale}"
    assert len(built) == len(rows)


def test_the_three_families_are_the_ones_the_table_parses():
    T = _T()
    assert {T.FAMILY_RE.match(r.symbol)["family"] for r in T.REG_INSTANTIATIONS} == set(FAMILIES)


def test_every_row_has_exactly_one_of_shapes_and_unreachable():
    T = _T()
    for r in T.REG_INSTANTIATIONS:
        assert not hasattr(r, "covered_by"), r.symbol   # no row points at another test: it runs, or no call can reach it
        assert sum(x is not None for x in (r.cases, r.unreachable)) == 1, r.symbol
        if r.cases is not None:
            assert r.kernels and r.markers, r.symbol
    # unreachable: only where the compiler-scheduled launcher (SCHED = 0, mfma_pipe) instantiates a descriptor kernel it never picks
    unreachable = [r for r in T.REG_INSTANTIATIONS if r.unreachable is not None]
    for r in unreachable:
        family, _, _, g = r.parsed
        assert family == "sgemm_mfma_kernel" and g["sched"] == "0", r.symbol
        assert re.match(r"csrc/\w+\.hip:\d+ ", r.unreachable), r.symbol
    assert len(unreachable) == 1, [r.symbol for r in unreachable]
    # ... and the line it names is the one that folds
    where = re.match(r"(csrc/\w+\.hip):(\d+) ", unreachable[0].unreachable)
    line = open(os.path.join(REPO, "how-to-optimize-gemm_amd", where[1])).read().splitlines()[int(where[2]) - 1]
    assert "BUFLD && win ? launch(sgemm_mfma_kernel<BM, BN, true, SCHED, 0, true" in line, line


def test_every_row_is_reached_the_way_it_says():
    import how_to_optimize_gemm_amd as H
    T = _T()
    for r in T.REG_INSTANTIATIONS:
        if r.cases is None:
            continue
        family, bm, bn, g = r.parsed
        _, _, kb = r.tile
        edge = g["edge"] == "true"
        sk = family == "sgemm_mfma_streamk_kernel"
        assert r.guarded == edge and ("guarded" in r.markers) == edge and ("guarded" in r.absent) == (not edge), r.symbol
        assert f"{family}<{bm},{bn}>" in r.markers, r.symbol
        assert r.streamk == (2 if sk else 0) and r.persist == (1 if sk else 0) and ("persistent" in r.markers) == sk, r.symbol
        assert sk or "persistent" in r.absent, r.symbol
        for kernel in r.kernels:
            assert kernel in H.KERNELS, (r.symbol, kernel)
        # the forced kernels are the ones whose launcher names this tile (mfma_tiles: the 128x128 tile without stream-K)
        if family == "sgemm_mfma_simple_kernel":
            assert r.kernels == ("mfma_simple",)
        elif g.get("sched") == "0":
            assert r.kernels == ("mfma_pipe",) and r.bufld is None
        else:
            tile = (bm, bn, int(g["wtn"]), int(g["wtm"]), kb)
            assert all(T.REG_TILES[k if k != "mfma_tiles" else "mfma"] == tile for k in r.kernels), r.symbol
            assert not sk or r.kernels[0] in T.SK_TILES, r.symbol
            assert r.bufld == (True if sk else g["bufld"] == "true"), r.symbol
        cases = r.cases(CUS)
        assert cases, r.symbol
        rounds = 0
        for c in cases:
            lda, ldb = r.leading_dimensions(c)
            # fast_shape's rule for the tile's KB; guarded rows also run whole-tile shapes: their odd leading dimensions
            # and 4-byte bases make them guarded
            whole = c.m % bm == 0 and c.n % bn == 0 and c.k % kb == 0 and lda % 4 == 0 and ldb % 4 == 0
            assert whole == (not edge) and (not edge or (lda % 2 == 1 and ldb % 2 == 1)), (r.symbol, c)
            assert lda >= c.k and ldb >= c.n, (r.symbol, c)
            # the window predicate picks this row's instantiation
            assert r.reached_by(c), (r.symbol, c)
            if r.bufld is not None:
                assert T.window_ok(bm, bn, c.k, lda, ldb) == r.bufld, (r.symbol, c)
            # a large operand fits the NaN buffer
            off = 1 if edge else 4
            if c.lda:
                assert off + (c.m - 1) * c.lda + c.k <= T.BIG_FLOATS and not c.ldb, (r.symbol, c)
            if c.ldb:
                assert off + (c.k - 1) * c.ldb + c.n <= T.BIG_FLOATS, (r.symbol, c)
            tiles = math.ceil(c.m / bm) * math.ceil(c.n / bn)
            if sk:
                w = T.per_cu_by_lds(bm, bn, kb)
                assert w >= 1 and tiles > CUS, (r.symbol, c)          # a persistent grid exists
                if c.whole_rounds:
                    rounds += 1
                    assert all(tiles % (v * CUS) == 0 and tiles >= 2 * v * CUS for v in range(1, w + 1)), (r.symbol, c)
                else:
                    assert all(tiles % (v * CUS) for v in range(1, w + 1)) and tiles < 2 * CUS, (r.symbol, c)   # ragged on every grid
                assert c.k > 2 * kb, (r.symbol, c)                    # K-slices to split
            else:
                assert not c.whole_rounds, (r.symbol, c)
        assert rounds == (1 if sk else 0), r.symbol
        inside = [c for c in cases if not c.lda and not c.ldb]
        if edge and not sk and inside:
            # the K-tail classes of the tile's own slices: none, 1, KB - 1, and a tail behind two and more whole slices
            tails = {c.k % kb for c in inside}
            assert {0, 1, kb - 1} <= tails, (r.symbol, tails)
            assert any(c.k > 2 * kb and c.k % kb for c in inside), r.symbol
            assert any(c.m % bm and c.n % bn for c in inside) and any(c.m < bm and c.n < bn for c in inside), r.symbol
        if not edge and not sk and inside:
            assert any(c.m > bm and c.n > bn and c.k >= 7 * kb for c in inside), r.symbol   # more than one block, a steady-state loop


def test_the_rows_beyond_the_window_cover_both_operands_of_every_tile():
    T = _T()
    for kernel in T.BEYOND_KERNELS:
        for guarded in (False, True):
            rows = [r for r in T.REG_INSTANTIATIONS if r.cases is not None and kernel in r.kernels and r.guarded == guarded and r.streamk == 0]
            beyond = [c for r in rows for c in r.cases(CUS) if c.lda or c.ldb]
            assert any(c.lda for c in beyond) and any(c.ldb for c in beyond), (kernel, guarded)
            bm, bn, kb = rows[0].tile
            smallest = past = 0
            for c in beyond:
                lda, ldb = rows[0].leading_dimensions(c)
                assert not T.window_ok(bm, bn, c.k, lda, ldb), (kernel, c)
                assert (c.m, c.n, c.k) == ((bm + 1, bn + 17, kb + 1) if guarded else (bm, bn, kb)), (kernel, c)
                # the smallest leading dimension that fails (one admissible step less is inside), or the smallest that puts
                # the operand's last row at byte offset 2^31
                step = 2 if guarded else 4
                if T.window_ok(bm, bn, c.k, lda - step if c.lda else lda, ldb - step if c.ldb else ldb):
                    smallest += 1
                else:
                    last = (c.m - 1) * c.lda if c.lda else (c.k - 1) * c.ldb
                    assert last * 4 >= 1 << 31 > (last - step * ((c.m if c.lda else c.k) - 1)) * 4, (kernel, c)
                    past += 1
            assert smallest == 2 and past == (0 if guarded else 2), (kernel, guarded, smallest, past)


def _plan(T, case, guarded):
    import how_to_optimize_gemm_amd as H
    name, _, _ = H.auto_plan(case.m, case.n, case.k, lda=case.lda or T._ld(case.k, guarded), ldb=case.ldb or T._ld(case.n, guarded),
                             ldc=T._ld(case.n, guarded), base_align=4 if guarded else 16, cu_count=CUS)
    return name


def test_window_ok_restated_agrees_with_the_library_at_the_boundary():
    """At the largest leading dimension the boundary test runs, mmh_auto_plan returns an LDS-DMA kernel; one admissible step
    beyond the 64x64 tiles' window -- the smallest tile of the LDS-DMA families, so every family's fails -- a register-staged
    one, fallback_kernel's.  (One step beyond a 128x128 tile's window the smaller families still take the shape.)"""
    T = _T()
    reg_names = {(128, 128): "mfma", (128, 64): "mfma_128x64", (64, 64): "mfma_64x64", (256, 256): "mfma_256x256"}
    flipped = 0
    for kernel, (bm, bn, kb, fallback) in T.BOUNDARY_KERNELS.items():
        for guarded, case in T.boundary_cases(kernel, 0):
            assert T._boundary_window(kernel, guarded, case), (kernel, case)
            assert (case.m, case.n, case.k) == T.boundary_shape(kernel, guarded)
            assert "_dma" in _plan(T, case, guarded), (kernel, case, _plan(T, case, guarded))
        for guarded, case in T.boundary_cases(kernel, 1):
            assert not T._boundary_window(kernel, guarded, case), (kernel, case)
            name = _plan(T, case, guarded)
            if T._boundary_window(kernel, guarded, case, T.SMALLEST_DMA_TILE):
                assert (bm, bn) != T.SMALLEST_DMA_TILE and "_dma" in name, (kernel, case, name)
            else:
                assert name == reg_names[T.fallback_tile(case.m, case.n, CUS)], (kernel, case, name)
                flipped += 1
    assert flipped >= 8, flipped   # both 64x64 ids, both operands, guarded and whole
    for kernel in T.FALLBACK_IDS:
        assert T.BOUNDARY_KERNELS[kernel][3] is not None and "_dma" in kernel


def test_the_operands_past_4_gib_keep_every_tile_inside_the_window():
    T = _T()
    assert 1024 in T.FAR_ROWS   # the shape the int8 suite's test_a_larger_than_4_gib_stays_in_place set: rows past byte offset 2^32
    for kernel, rows, streamk in T.FAR_CASES:
        bm, bn, k = T.FAR_KERNELS[kernel]
        m, n, kk = T.far_shape(kernel, rows, streamk, CUS)
        assert m <= T.FAR_MAX_ROWS and m == rows + bm + 1 and kk == k
        assert (m - 1) * T.FAR_LD * 4 >= 1 << 32                    # the last tile row of A and C lies past byte offset 2^32
        assert rows < 2048 or (m - 1) * T.FAR_LD >= 1 << 31         # ... and, from 2048 rows, past element offset 2^31
        assert T.window_ok(bm, bn, k, T.FAR_LD, n)
        tiles = math.ceil(m / bm) * math.ceil(n / bn)
        if streamk:
            assert kernel in T.FAR_STREAMK and CUS < tiles < 2 * CUS and tiles % CUS, (kernel, tiles)
        else:
            assert n == bn + 1
    assert {(k, r) for k, r, s in T.FAR_CASES if not s} == {(k, r) for k in T.FAR_KERNELS for r in T.FAR_ROWS}
