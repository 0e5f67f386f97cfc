"""Every LDS-DMA fp32 GEMM instantiation in the built product library has a row in the oracle parity table
(tests/test_gpu_lds_dma_parity.py::INSTANTIATIONS), and every row names an instantiation that is there -- read on the CPU
from the library's code objects (tools/kernel_resources.py).  A tile family that ships without a row fails here, by name,
before anything runs on a GPU.  The rows' shapes are checked here too, on the host arithmetic the launchers use: that
each one reaches its row's instantiation (whole or guarded, ragged or whole-round tile counts)."""
import math
import re

import built_lib

pytestmark = built_lib.needs_library

FAMILIES = ("sgemm_mfma_dma_kernel", "sgemm_dma_streamk_kernel", "sgemm_mfma_dma5_kernel", "sgemm_dma5_streamk_kernel",   # K2L, K2W
            "sgemm_valu_dma5_kernel", "sgemm_valu_dma5_streamk_kernel",                                                 # K1W
            "sgemm_mfma_dma5_op_kernel", "sgemm_dma5_op_streamk_kernel")                                                # op forms
FAMILY = re.compile(r"^(" + "|".join(FAMILIES) + r")<")
CUS = 256   # the MI355X's compute units (the GPU test derives its shapes from the device's count)


def _table():
    from test_gpu_lds_dma_parity import FAMILY_RE, INSTANTIATIONS
    return FAMILY_RE, INSTANTIATIONS


def test_the_table_names_every_lds_dma_instantiation_of_the_library():
    _, rows = _table()
    symbols = [r.symbol for r in rows]
    assert len(symbols) == len(set(symbols)), "a symbol has two rows"
    built = built_lib.built(FAMILY)
    missing = sorted(built - set(symbols))
    stale = sorted(set(symbols) - built)
    assert not missing, f"instantiations in libmmult_hip.so without a row in INSTANTIATIONS: {missing}"
    assert not stale, f"rows of INSTANTIATIONS that name no instantiation of libmmult_hip.so: {stale}"
    assert len(built) == 79, len(built)


def test_the_eight_families_are_the_ones_the_table_parses():
    family_re, rows = _table()
    assert {family_re.match(r.symbol)["family"] for r in rows} == set(FAMILIES)


def test_every_row_is_reached_the_way_it_says():
    import how_to_optimize_gemm_amd as H
    _, rows = _table()
    for r in rows:
        bm, bn = r.bm_bn
        guarded = "guarded" in r.markers
        sk = "persistent" in r.markers
        assert r.kernel in H.KERNELS, r
        assert r.streamk == (2 if sk else 0) and r.persist == (1 if sk else 0), r
        assert ("chained parts" in r.absent) == (r.chain == 0), r
        assert r.ops is None or f"operands {'NT'[r.ops[0]]}{'NT'[r.ops[1]]}" in r.markers, r
        shapes = r.shapes(CUS)
        assert shapes, r
        rounds = 0
        for m, n, k, whole_rounds in shapes:
            whole = m % bm == 0 and n % bn == 0 and k % 32 == 0
            tiles = math.ceil(m / bm) * math.ceil(n / bn)
            # guarded rows also run whole-tile shapes: their odd leading dimensions and 4-byte bases make them guarded
            assert guarded or whole, (r.symbol, m, n, k)
            if r.tiles_ok is not None:
                assert r.tiles_ok(tiles, CUS), (r.symbol, m, n, k)
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
            if "dma5" in r.symbol:   # K2W: thin last tile rows / columns of 1, 15, 16 and 17
                thin = {m - (math.ceil(m / bm) - 1) * bm for m, _, _, _ in shapes if m > bm} | \
                       {n - (math.ceil(n / bn) - 1) * bn for _, n, _, _ in shapes if n > bn}
                assert {1, 15, 16, 17} <= thin, (r.symbol, thin)


def test_the_auto_shapes_are_planned_on_the_odd_blocked_tiles():
    import how_to_optimize_gemm_amd as H
    from test_gpu_lds_dma_parity import AUTO_SHAPES
    picks = {H.auto_plan(m, n, k, cu_count=CUS)[0] for m, n, k in AUTO_SHAPES}
    assert picks == {"mfma_96x64_dma5", "mfma_160x160_dma5"}, picks
