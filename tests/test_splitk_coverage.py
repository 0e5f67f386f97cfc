"""Every instantiation of the opt-in split-K kernel (sgemm_mfma_splitk_kernel) in the built product library has a row in
tests/test_gpu_splitk_parity.py::SPLITK_INSTANTIATIONS, and every row names an instantiation that is there -- read on the CPU
from the library's code objects (tools/kernel_resources.py).  The rows are held to the catalogue (csrc/abi.hip: the two ids whose
launcher is Launcher::SplitK, each on its fall-back tile) and to csrc/launch_reg.hip's two instantiations, and every case is
proved here, on the launcher's host arithmetic, to split: whole tiles, at least two parts, and -- the residency case aside --
every part resident on any device, so that the part count is the restated one."""
import os
import re

import pytest

import built_lib
import kernel_tables as R

CSRC = os.path.join(built_lib.REPO, "how-to-optimize-gemm_amd", "csrc")
pytestmark = built_lib.needs_library

FAMILY = re.compile(r"^sgemm_mfma_splitk_kernel<")
CUS = 256   # the MI355X's compute units (the GPU test derives its shapes from the device's count)
ALL_CUS = (CUS, 304, 64)


def _T():
    import test_gpu_splitk_parity as T
    return T


def test_the_table_names_every_split_k_instantiation_of_the_library():
    rows = _T().SPLITK_INSTANTIATIONS
    symbols = [r.symbol for r in rows]
    assert len(symbols) == len(set(symbols)), "a symbol has two rows"
    built = built_lib.built(FAMILY)
    missing = sorted(built - set(symbols))
    stale = sorted(set(symbols) - built)
    assert not missing, f"instantiations in libmmult_hip.so without a row in SPLITK_INSTANTIATIONS: {missing}"
    assert not stale, f"rows of SPLITK_INSTANTIATIONS that name no instantiation of libmmult_hip.so: {stale}"
    assert len(built) == 2, len(built)


def test_the_rows_are_the_catalogues_split_k_ids_on_their_tiles():
    import how_to_optimize_gemm_amd as H
    T = _T()
    abi = open(os.path.join(CSRC, "abi.hip")).read()
    catalogue = re.findall(r'\{MMH_KERNEL_(\w+), "MMult_hip_(\w+)", Launcher::SplitK, MMH_KERNEL_(\w+)\}', abi)
    assert sorted(name for _, name, _ in catalogue) == sorted(r.kernel for r in T.SPLITK_INSTANTIATIONS)
    launch = open(os.path.join(CSRC, "launch_reg.hip")).read()
    assert "return tile == MMH_KERNEL_MFMA_128X64 ? try_launch_splitk<128, 64, 2>(ctx, S, g) : try_launch_splitk<128, 128, 4>(ctx, S, g);" in launch
    assert "template <int BM, int BN, int WTN, int WTM = 4, int KB = BK>\nint try_launch_splitk(" in launch
    fallback = {name: tile.lower() for _, name, tile in catalogue}       # id -> the register-staged tile it runs on
    for r in T.SPLITK_INSTANTIATIONS:
        assert r.kernel in H.KERNELS and r.kernel not in H.CHAIN_KERNELS, r.symbol
        g = T.FAMILY_RE.match(r.symbol)
        tile = tuple(int(g[x]) for x in ("bm", "bn", "wtn", "wtm", "kb"))
        assert R.REG_TILES[fallback[r.kernel]] == tile and tile[4] == T.KB, (r.symbol, fallback[r.kernel])
        assert f"try_launch_splitk<{tile[0]}, {tile[1]}, {tile[2]}>" in launch, r.symbol


@pytest.mark.parametrize("cus", ALL_CUS)
def test_every_case_splits_the_way_it_says(cus):
    T = _T()
    for r in T.SPLITK_INSTANTIATIONS:
        bm, bn, kb = r.tile
        cases = r.cases(cus)
        names = [c.what for c in cases]
        for what in ("smallest split", "uneven parts", "uneven boundaries", "first clamp", "several tiles", "chosen part count",
                     "residency clamp"):
            assert what in names, (r.symbol, what)
        assert any(c.auto for c in cases) == ((bm, bn) == (128, 128)), r.symbol      # MMH_KERNEL_AUTO splits on the 128x128 tile only
        for c in cases:
            tile = (128, 128) if c.auto else (bm, bn)
            # try_launch_splitk: fast_shape (run_gemm's operands are aligned, their leading dimensions multiples of 4), the window
            assert c.m % tile[0] == 0 and c.n % tile[1] == 0 and c.k % kb == 0, (r.symbol, c)
            assert R.window_ok(*tile, c.k, T._ld(c.k, False), T._ld(c.n, False)) and T._ld(c.k, False) % 4 == 0 and T._ld(c.n, False) % 4 == 0
            tiles = (c.m // tile[0]) * (c.n // tile[1])
            S = T.expected_parts(c, *tile, cus)
            assert 2 <= S <= c.k // kb, (r.symbol, c, S)
            if c.auto:      # policy.hip sgemm_on: fewer 128x128 (and 256x256) tiles than CUs, the option set
                assert c.requested >= 1 and tiles < cus, (r.symbol, c)
            else:
                assert c.requested != 1, (r.symbol, c)
            if c.residency:
                w = R.per_cu_by_lds(*tile, kb)
                left = T.residency_counts(*tile, cus, tiles)
                # the clamp bites whatever the registers allow, and two parts are resident at one workgroup per CU
                assert c.requested == 8 and S == 8 and tiles * 8 > w * cus and tiles * 2 <= cus, (r.symbol, c)
                assert all(2 <= s < 8 for s in left), (r.symbol, c, left)
            else:
                assert tiles * S <= cus, (r.symbol, c)      # resident at one workgroup per CU: the clamp is idle
            assert 2 * c.m * c.n * c.k <= 2e9, (r.symbol, c)   # the oracle's work per restatement
        by = {c.what: c for c in cases if not c.auto}
        assert (by["smallest split"].k, by["smallest split"].requested) == (64, 2)
        assert T.expected_parts(by["first clamp"], bm, bn, cus) == 3 and by["first clamp"].requested == 8
        assert T.ref.boundaries(by["uneven parts"].k // kb, 2) == [0, 1, 3]
        assert T.ref.boundaries(by["uneven boundaries"].k // kb, by["uneven boundaries"].requested) == [0, 1, 3, 5, 7]
        assert (by["several tiles"].m, by["several tiles"].n) == (2 * bm, 3 * bn)
        assert [T.expected_parts(c, bm, bn, cus) for c in cases if c.what == "chosen part count"] == [2, 4, 8]
        assert [T.expected_parts(c, 128, 128, cus) for c in cases if c.auto] == ([2, 4, 8, 4] if (bm, bn) == (128, 128) else [])


def test_the_shared_shape_and_the_stream_k_rows_it_is_interleaved_with():
    """6 tiles of 128x128 (12 of 128x64), 7 K-slices; the stream-K steps are the first shapes of two existing rows."""
    T = _T()
    m, n, k = T.SHARED_SHAPE
    assert (m // 128) * (n // 128) == 6 and k // T.KB == 7 and m % 128 == 0 and n % 128 == 0
    (reg, reach), (k2w, _) = T._streamk_rows()
    assert reg.streamk == 2 and reach.kernel == "mfma" and k2w.streamk == 2 and k2w.kernel == "mfma_128x128_dma5"
    # ... as the two tables have them: the same reach, the same proof, the same first shape
    from test_gpu_lds_dma_parity import INSTANTIATIONS
    from test_gpu_reg_parity import REG_INSTANTIATIONS
    reg_row = next(r for r in REG_INSTANTIATIONS if r.symbol == reg.symbol)
    k2w_row = next(r for r in INSTANTIATIONS if r.symbol == k2w.symbol)
    assert (reg_row.kernels[0], reg_row.streamk, reg_row.persist, reg_row.markers) == (reg.kernel, reg.streamk, reg.persist, reg.markers)
    assert (k2w_row.kernel, k2w_row.streamk, k2w_row.chain, k2w_row.persist) == (k2w.kernel, k2w.streamk, k2w.chain, k2w.persist)
    assert k2w_row.markers == k2w.markers and k2w_row.ops is None and not reg_row.guarded, (k2w_row, reg_row)
    for cus in ALL_CUS:
        c = reg_row.cases(cus)[0]
        assert ((c.m, c.n, c.k), k2w_row.shapes(cus)[0][:3]) == T.streamk_shapes(cus) and not c.lda and not c.ldb, cus
    for cus in ALL_CUS:
        for shape in T.streamk_shapes(cus):
            tiles = (shape[0] // 128) * (shape[1] // 128)
            assert cus < tiles < 2 * cus and 2 * shape[0] * shape[1] * shape[2] <= 2e9, (cus, shape)
