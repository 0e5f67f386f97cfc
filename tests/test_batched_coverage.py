"""Every plain batched instantiation in the built product library has a row in
tests/test_gpu_batched_parity.py::BATCHED_INSTANTIATIONS, and every row names an instantiation that is there -- read on the CPU
from the library's code objects (tools/kernel_resources.py).  The rows' shapes are checked here too, on the host arithmetic the
launcher uses (dma5_form, csrc/internal.hpp, as tests/kernel_tables.py restates it): that each one reaches its row's
instantiation, whole or guarded, and the classes the table claims; and the shapes of the tail-split, per == 3 and special-value
tests of that module."""
import math
import re

import built_lib
from kernel_tables import TILES, _special_shapes, _whole, tail_split, tail_split_case

pytestmark = built_lib.needs_library

FAMILY = re.compile(r"^sgemm_mfma_dma5_batched_kernel<")
CUS = 256   # the MI355X's compute units (the GPU test derives its tail-split batch from the device's count)


def _T():
    import test_gpu_batched_parity as T
    return T


def test_the_table_names_every_batched_instantiation_of_the_library():
    symbols = [r.symbol for r in _T().BATCHED_INSTANTIATIONS]
    assert len(symbols) == len(set(symbols)), "a symbol has two rows"
    built = built_lib.built(FAMILY)
    missing = sorted(built - set(symbols))
    stale = sorted(set(symbols) - built)
    assert not missing, f"instantiations in libmmult_hip.so without a row in BATCHED_INSTANTIATIONS: {missing}"
    assert not stale, f"rows of BATCHED_INSTANTIATIONS that name no instantiation of libmmult_hip.so: {stale}"
    assert len(built) == 24, len(built)


def test_the_rows_spell_their_symbols_as_the_resource_test_does():
    from test_batched_kernel_resources import _twins
    assert {r.symbol for r in _T().BATCHED_INSTANTIATIONS} == {b for b, _, _ in _twins()}


def test_no_row_is_an_escape_hatch():
    """All 24 are reachable through mmh_sgemm_batched with a forced tile: every row runs cases, none points elsewhere."""
    for r in _T().BATCHED_INSTANTIATIONS:
        assert not hasattr(r, "covered_by") and not hasattr(r, "unreachable"), r.symbol
        assert r.cases(), r.symbol


def _thin(x, tile):
    return x - (math.ceil(x / tile) - 1) * tile


def test_every_row_is_reached_the_way_it_says():
    import how_to_optimize_gemm_amd as H
    T = _T()
    for r in T.BATCHED_INSTANTIATIONS:
        g = T.FAMILY_RE.match(r.symbol)
        assert g, r.symbol
        assert (r.bm, r.bn) == (int(g["bm"]), int(g["bn"])) and r.guarded == (g["edge"] == "true"), r
        assert r.kernel == f"mfma_{r.bm}x{r.bn}_dma5" and r.kernel in H.KERNELS, r
        assert r.ops == (int(g["op"]) & 1, int(g["op"]) >> 1), r
        cases = r.cases()
        for m, n, k, batch, extra in cases:
            assert batch == 3, (r.symbol, batch)
            # dma5_form: whole tiles, multiples of 4, 16-byte bases and strides -- or not
            assert _whole(r.bm, r.bn, *r.ops, m, n, k, batch, extra) == (not r.guarded), (r.symbol, m, n, k, extra)
            # every matrix has operands of its own, at least the packed matrix apart, and the C matrices do not overlap
            ra, ca, rb, cb = T.stored(r.ops, m, n, k)
            ldc = extra.get("ldc") or n
            assert extra["sa"] >= ra * ca and extra["sb"] >= rb * cb and extra["sc"] >= (m - 1) * ldc + n, (r.symbol, extra)
        if r.guarded:
            assert {(m, n, k) for m, n, k, _, _ in cases} == {(129, 143, 77), (144, 145, 33)}, r.symbol
            assert all(k % 32 for _, _, k, _, _ in cases), r.symbol   # both have a K tail
            # the thin last tile rows / columns (<= 16 takes the written-out raster's thin_row / thin_col branches, 17 does not)
            thin = {_thin(m, r.bm) for m, _, _, _, _ in cases if m > r.bm} | {_thin(n, r.bn) for _, n, _, _, _ in cases if n > r.bn}
            assert {1, 15, 16, 17} <= thin, (r.symbol, thin)
            # BOTH thin at once in one case (n_full = (nbm - 1) (nbn - 1); the thin column's tiles come before the thin row's)
            assert any(m > r.bm and n > r.bn and _thin(m, r.bm) <= 16 and _thin(n, r.bn) <= 16 for m, n, _, _, _ in cases), r.symbol
            odd = [e for _, _, _, _, e in cases if all(e[s] % 4 for s in ("sa", "sb", "sc")) and all(o % 4 for o in e.get("offs", (0,)))]
            assert odd, (r.symbol, "no case with every stride and base off the 16-byte grid")
        else:
            assert [(m, n, k) for m, n, k, _, _ in cases] == [(2 * r.bm, 3 * r.bn, 96)], r.symbol
            m, n, k, _, extra = cases[0]
            nbm, nbn = m // r.bm, n // r.bn
            assert nbm > 1 and nbn > 1 and nbm != nbn and k // 32 == 3, r.symbol   # the (matrix, tile) split, three K-slices
            assert extra["ldc"] == n + 4 and extra["sc"] > m * extra["ldc"] and extra["sa"] % 4 == 0 and extra["sb"] % 4 == 0
            ra, ca, rb, cb = T.stored(r.ops, m, n, k)
            assert extra["sa"] > ra * ca and extra["sb"] > rb * cb, (r.symbol, "no gap between the matrices")


def test_the_planner_names_a_kernel_for_every_rows_shapes():
    import how_to_optimize_gemm_amd as H
    for r in _T().BATCHED_INSTANTIATIONS:
        for m, n, k, batch, extra in r.cases():
            name, form, wgs = H.auto_plan_batched(*r.ops, m, n, k, ldc=extra.get("ldc", 0), stride_a=extra["sa"], stride_b=extra["sb"],
                                                  stride_c=extra["sc"], batch=batch, base_align=4 if r.guarded else 16, cu_count=CUS)
            assert name in H.KERNELS and form in H.BATCH_FORMS.values() and wgs >= batch, (r.symbol, m, n, k, name, form, wgs)


def test_the_tail_split_case_splits_on_the_launchers_rule():
    """dma5_split_first gives the first launch 3 CUs workgroups; the second one's ids start there: the last quarter of the batch."""
    T = _T()
    for cus in (CUS, 304, 64):
        m, n, k, batch = tail_split_case(cus)
        per = math.ceil(m / 64) * math.ceil(n / 64)
        tiles = batch * per
        assert tail_split(tiles, 3, cus, k) and tiles <= (1 << 22)
        first = 3 * cus
        assert first % per == 0 and first // per == batch - batch // 4 and (tiles - first) // per == batch // 4
        assert m % 64 == 0 and n % 64 == 0 and k % 32 == 0 and (m * k) % 4 == 0 and (m * n) % 4 == 0   # whole: no "guarded"
    for sa, sb, accumulate in T.SPLIT_RUNS.values():
        # what tells the matrices apart: an A per matrix, or (accumulate) the C the chain starts from
        assert sb == 0 and ((sa is None and not accumulate) or (sa == 0 and accumulate))


def test_the_per_3_case_leaves_a_first_launch_that_is_no_multiple_of_8():
    import how_to_optimize_gemm_amd as H
    T = _T()
    p = T.PER3
    cap = H.BATCHED_MAX_WORKGROUPS
    per = math.ceil(p["m"] / 64) * math.ceil(p["n"] / 64)
    assert per == 3 and cap % per != 0                        # whole matrices per launch: cap // 3 of them
    assert (cap // 3) * 3 % 8 != 0 and (cap // 3) * 3 == 4194303
    batch = T.per3_batch(cap)
    mats = cap // per
    assert mats < batch <= 2 * mats and batch - mats == 2      # two launches, the second of two matrices
    assert p["sc"] >= (p["m"] - 1) * p["ldc"] + p["n"], "the C matrices overlap"
    assert p["sa"] == 0 and p["sb"] >= 1 and p["lda"] >= p["k"] and p["ldb"] >= p["n"]
    assert 0.7e9 < batch * p["sc"] * 4 < 0.75e9                # C: about 0.72 GB
    assert _thin(p["m"], 64) == 1                              # a thin last tile row


def test_the_special_shapes_are_whole_and_guarded_on_every_tile(oracle):
    T = _T()
    assert [t for t, _ in T.SPECIAL_CASES[::4]] == TILES and len(T.SPECIAL_CASES) == 12
    for kernel in TILES:
        bm, bn = (int(x) for x in re.search(r"_(\d+)x(\d+)", kernel).groups())
        (wm, wn, wk, wg), (gm, gn, gk, gg) = _special_shapes(kernel)
        assert wm % bm == 0 and wn % bn == 0 and wk % 32 == 0 and not wg, kernel
        assert gg and gk % 32 and (gm % bm or gn % bn), kernel
    # the blocks' layout and expectations, on the smallest tile's two shapes and the NT pair (the oracle's CPU library is all this needs)
    for m, n, k, guarded in _special_shapes("mfma_64x64_dma5"):
        bt, neg_zero = T.special_batch(oracle, (0, 1), m, n, k, guarded)
        assert bt.batch == 4 and bt.sa and bt.sb and bt.sc >= (m - 1) * bt.ldc + n
        whole = all(x % 4 == 0 for x in (bt.lda, bt.ldb, bt.ldc, bt.sa, bt.sb, bt.sc) + tuple(bt.offs))
        assert whole == (not guarded), (m, n, k)
        for accumulate in (False, True):
            T.check_special_expectation([bt.want(oracle, i, accumulate) for i in range(4)], neg_zero, accumulate)
