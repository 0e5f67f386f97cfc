"""Every batched fused-epilogue instantiation in the built product library has a row in
tests/test_gpu_batched_ex.py::BATCHED_EX_INSTANTIATIONS, and every row names an instantiation that is there -- read on the CPU
from the library's code objects (tools/kernel_resources.py).  The rows' shapes are checked here too, on the host arithmetic the
launcher uses (dma5_form, csrc/internal.hpp): that each one reaches its row's instantiation, whole or guarded, and what the
guarded ones cover; and the shapes of the tail-split, loop and special-value tests."""
import math
import re

import built_lib
from kernel_tables import _special_shapes, _whole

pytestmark = built_lib.needs_library

FAMILY = re.compile(r"^sgemm_mfma_dma5_batched_ex_kernel<")
CUS = 256   # the MI355X's compute units (the GPU test derives its tail-split batch from the device's count)


def _rows():
    from test_gpu_batched_ex import BATCHED_EX_INSTANTIATIONS
    return BATCHED_EX_INSTANTIATIONS


def test_the_table_names_every_batched_ex_instantiation_of_the_library():
    symbols = [r.symbol for r in _rows()]
    assert len(symbols) == len(set(symbols)), "a symbol has two rows"
    built = built_lib.built(FAMILY)
    missing = sorted(built - set(symbols))
    stale = sorted(set(symbols) - built)
    assert not missing, f"instantiations in libmmult_hip.so without a row in BATCHED_EX_INSTANTIATIONS: {missing}"
    assert not stale, f"rows of BATCHED_EX_INSTANTIATIONS that name no instantiation of libmmult_hip.so: {stale}"
    assert len(built) == 24, len(built)


def test_the_rows_spell_their_symbols_as_the_resource_test_does():
    from test_batched_ex_kernel_resources import _twins
    assert {r.symbol for r in _rows()} == {b for b, _, _ in _twins()}


def test_every_row_is_reached_the_way_it_says():
    import how_to_optimize_gemm_amd as H
    from test_gpu_batched_ex import FAMILY_RE
    for r in _rows():
        g = FAMILY_RE.match(r.symbol)
        assert g, r.symbol
        assert (r.bm, r.bn) == (int(g["bm"]), int(g["bn"])) and r.guarded == (g["edge"] == "true"), r
        assert r.kernel == f"mfma_{r.bm}x{r.bn}_dma5" and r.kernel in H.KERNELS, r
        assert r.ops == (int(g["op"]) & 1, int(g["op"]) >> 1), r
        cases = r.cases()
        assert cases, r
        for m, n, k, batch, extra in cases:
            assert 3 <= batch <= 6, (r.symbol, batch)
            assert _whole(r.bm, r.bn, *r.ops, m, n, k, batch, extra) == (not r.guarded), (r.symbol, m, n, k, extra)
            sc = extra.get("sc", m * (extra.get("ldc") or n))
            assert sc >= (m - 1) * (extra.get("ldc") or n) + n, (r.symbol, "the C matrices overlap")
        if r.guarded:
            assert any(k % 32 for _, _, k, _, _ in cases), r.symbol   # a K tail
            thin = {m - (math.ceil(m / r.bm) - 1) * r.bm for m, _, _, _, _ in cases if m > r.bm} | \
                   {n - (math.ceil(n / r.bn) - 1) * r.bn for _, n, _, _, _ in cases if n > r.bn}
            assert {1, 15, 16, 17} <= thin, (r.symbol, thin)
            assert any(e.get("sc", 0) % 4 for _, _, _, _, e in cases) and any(any(o % 4 for o in e.get("offs", ())) for _, _, _, _, e in cases)
        else:
            assert all(math.ceil(m / r.bm) * math.ceil(n / r.bn) > 1 for m, n, _, _, _ in cases), r.symbol   # several tiles per matrix


def test_the_planner_takes_every_rows_shapes_in_one_launch():
    import how_to_optimize_gemm_amd as H
    for r in _rows():
        for m, n, k, batch, extra in r.cases():
            ra, ca = (k, m) if r.ops[0] else (m, k)
            name, form, wgs = H.auto_plan_batched_ex(*r.ops, m, n, k, ldc=extra.get("ldc", 0), stride_c=extra.get("sc", -1), batch=batch,
                                                     bias_mode=1, stride_bias=n + 1, base_align=4 if r.guarded else 16, cu_count=CUS)
            assert form == "one_launch" and name in H.KERNELS and wgs >= batch, (r.symbol, m, n, k, name, form, wgs)


def test_the_tail_split_case_splits_on_the_launchers_rule():
    from test_gpu_batched_ex import tail_split, tail_split_case
    for cus in (CUS, 304, 64):
        m, n, k, batch = tail_split_case(cus)
        tiles = batch * math.ceil(m / 64) * math.ceil(n / 64)
        assert tail_split(tiles, 3, cus, k) and tiles - 3 * cus == cus and k == 512
    # dma5_tail_split, restated: one whole round, a last round of just under a tile per CU, k >= 512, a first launch of a multiple of 8
    assert not tail_split(4 * CUS, 3, CUS, 480) and not tail_split(4 * CUS + 1, 3, CUS, 512) and not tail_split(4 * CUS, 1, CUS, 512)
    assert tail_split(3 * CUS + 218, 3, CUS, 512) and not tail_split(3 * CUS + 217, 3, CUS, 512)


def test_the_special_shapes_are_whole_and_guarded_on_every_tile():
    from test_gpu_batched_ex import TILES
    for kernel in TILES:
        bm, bn = (int(x) for x in re.search(r"_(\d+)x(\d+)", kernel).groups())
        (wm, wn, wk, wg), (gm, gn, gk, gg) = _special_shapes(kernel)
        assert wm % bm == 0 and wn % bn == 0 and wk % 32 == 0 and not wg, kernel
        assert gg and gk % 32 and (gm % bm or gn % bn), kernel
        for m, n, k in ((wm, wn, wk), (gm, gn, gk)):
            assert m > 70 and n > 100 and k > 20, (kernel, m, n, k)   # (what special_blocks plants its values in)
