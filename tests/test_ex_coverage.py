"""Every fused-epilogue instantiation in the built product library has a row in tests/test_gpu_ex_parity.py::EX_INSTANTIATIONS,
and every row names an instantiation that is there -- read on the CPU from the library's code objects
(tools/kernel_resources.py).  An `ex` kernel that ships without a row fails here, by name, before anything runs on a GPU.
The rows' shapes are checked here too, on the host arithmetic the launchers use: that each one reaches its row's
instantiation (whole or guarded, ragged or whole-round tile counts) and that mmh_auto_plan_ex takes it.  The special-value
blocks of that file are built here as well, and each one's expectation is held to contain the class of values it is there
for (the oracle's CPU library is all this needs)."""
import math
import re

import built_lib

pytestmark = built_lib.needs_library

FAMILY = re.compile(r"^sgemm_(mfma_dma5_ex|dma5_ex_streamk)_kernel<")
CUS = 256   # the MI355X's compute units (the GPU test derives its shapes from the device's count)


def _rows():
    from test_gpu_ex_parity import EX_INSTANTIATIONS
    return EX_INSTANTIATIONS


def test_the_table_names_every_ex_instantiation_of_the_library():
    symbols = [r.symbol for r in _rows()]
    assert len(symbols) == len(set(symbols)), "a symbol has two rows"
    built = built_lib.built(FAMILY)
    missing = sorted(built - set(symbols))
    stale = sorted(set(symbols) - built)
    assert not missing, f"instantiations in libmmult_hip.so without a row in EX_INSTANTIATIONS: {missing}"
    assert not stale, f"rows of EX_INSTANTIATIONS that name no instantiation of libmmult_hip.so: {stale}"
    assert len(built) == 48, len(built)


def test_the_rows_spell_their_symbols_as_the_resource_test_does():
    from test_ex_kernel_resources import _twins
    assert {r.symbol for r in _rows()} == {ex for ex, _, _ in _twins()}


def test_every_row_is_reached_the_way_it_says():
    import how_to_optimize_gemm_amd as H
    from test_gpu_ex_parity import EX_FAMILY_RE, ROW_EPILOGUES, ex_tag
    # (the text tests/test_gpu_ex.py::test_stream_k_ex_launches_happen holds the library to, and the two other row epilogues')
    assert [ex_tag((0, 1), *e) for e in ROW_EPILOGUES.values()] == [", operands NT, epilogue alpha beta bias(col) relu",
                                                                    ", operands NT, epilogue bias(row)", ", operands NT, epilogue identity"]
    for r in _rows():
        bm, bn = r.bm_bn
        g = EX_FAMILY_RE.match(r.symbol)
        sk = "streamk" in g["family"]
        guarded = g["edge"] == "true"
        assert r.kernel == f"mfma_{bm}x{bn}_dma5" and r.kernel in H.KERNELS, r
        assert r.streamk == (2 if sk else 0) and r.persist == (1 if sk else 0), r
        assert r.ops == (int(g["op"]) & 1, int(g["op"]) >> 1), r
        assert r.head == f"{g['family']}<{bm},{bn}>", r
        assert r.guarded == guarded, r
        for word in ("persistent", "chained parts"):
            assert (word in r.markers) == sk and (word in r.absent) == (not sk), r
        assert ("guarded" in r.absent) == (not guarded), r
        shapes = r.shapes(CUS)
        assert shapes, r
        rounds = 0
        for m, n, k, whole_rounds in shapes:
            whole = m % bm == 0 and n % bn == 0 and k % 32 == 0
            tiles = math.ceil(m / bm) * math.ceil(n / bn)
            # guarded rows also run whole-tile shapes: their odd leading dimensions and 4-byte bases make them guarded
            assert guarded or whole, (r.symbol, m, n, k)
            if sk:
                assert tiles > CUS, (r.symbol, m, n, k)          # a persistent grid exists
                if whole_rounds:
                    rounds += 1
                    assert tiles % (6 * CUS) == 0, (r.symbol, m, n, k)
                else:
                    assert all(tiles % (w * CUS) for w in (1, 2, 3)), (r.symbol, m, n, k)   # ragged on every grid
        assert rounds == (1 if sk else 0), r.symbol
        if guarded and not sk:
            assert any(k % 32 for _, _, k, _ in shapes), r.symbol   # a K tail
            thin = {m - (math.ceil(m / bm) - 1) * bm for m, _, _, _ in shapes if m > bm} | \
                   {n - (math.ceil(n / bn) - 1) * bn for _, n, _, _ in shapes if n > bn}
            assert {1, 15, 16, 17} <= thin, (r.symbol, thin)


def test_the_ex_planner_takes_every_rows_shapes():
    import how_to_optimize_gemm_amd as H
    for r in _rows():
        for m, n, k, _ in r.shapes(CUS):
            for align in (4, 16):
                name, tiles, _ = H.auto_plan_ex(*r.ops, m, n, k, base_align=align, cu_count=CUS)
                assert name in H.KERNELS and tiles >= 1, (r.symbol, m, n, k, align, name, tiles)


def _special_shapes():
    from test_gpu_ex_parity import SPECIAL_TILES, special_shapes
    return sorted({(m, n, k) for kernel in ("naive",) + SPECIAL_TILES for m, n, k, _, _ in special_shapes(kernel, CUS)})


def test_the_special_shapes_are_whole_guarded_and_ragged_stream_k():
    from test_gpu_ex_parity import SPECIAL_TILES, special_shapes
    for kernel in SPECIAL_TILES:
        bm, bn = (int(x) for x in re.search(r"_(\d+)x(\d+)", kernel).groups())
        (wm, wn, wk, wg, ws), (gm, gn, gk, gg, gs), (sm, sn, s_k, sg, ss) = special_shapes(kernel, CUS)
        assert wm % bm == 0 and wn % bn == 0 and wk % 32 == 0 and not wg and not ws, kernel
        assert gg and not gs and gk % 32 and (gm % bm or gn % bn), kernel
        tiles = math.ceil(sm / bm) * math.ceil(sn / bn)
        assert sg and ss and s_k % 32 and tiles > CUS and all(tiles % (w * CUS) for w in (1, 2, 3)), kernel
    assert [s[3:] for s in special_shapes("naive", CUS)] == [(False, False), (True, False)]


def test_the_special_value_blocks_reach_their_classes(oracle):
    from test_gpu_ex_parity import special_blocks
    names = None
    for m, n, k in _special_shapes():
        blocks = special_blocks(oracle, m, n, k)
        assert names in (None, [b.name for b in blocks])
        names = [b.name for b in blocks]
        assert len(set(names)) == len(names) == 10, names
        for blk in blocks:
            assert blk.want.shape == (m, n) and blk.want.dtype.name == "float32", (m, n, k, blk.name)
            try:
                blk.check_expectation()
            except AssertionError as e:
                raise AssertionError(f"{(m, n, k)} {blk.name}: the expectation does not hold what the block is there for") from e
