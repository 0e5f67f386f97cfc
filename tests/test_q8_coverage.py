"""The case table of the int8 linear layer's GPU tests (tests/test_gpu_qlinear.py: Row.cases, gemm_cases, quant_cases) has the
classes it promises, checked on the CPU with the plan's Python restatement (tests/qlinear_ref.py: plan_text, big_tile) at the
MI355X's 256 compute units: every case reaches its row's instantiation; K depths with one to four trips of the tile's loop --
the first trip only consumes the prologue's two slices, so it takes more than 256 columns to refill an LDS buffer inside the
loop -- and every K tail; thin last tiles in both directions; odd leading dimensions and bases past alignment; grids that are
no multiple of the 8 XCDs, one tile row and one tile column; the row quantiser's two forms on both paths with columns behind
the last float4 on both sides of what the wide form keeps in LDS.  A kernel change that drops a class from the table fails here."""
import math

import pytest

import built_lib
import qlinear_ref as R
import test_gpu_qlinear as T

CUS = 256   # the MI355X's compute units (the GPU test derives its shapes from the device's count)
GEMM_ROWS = [r for r in T.Q8_INSTANTIATIONS if r.kind == "gemm"]
QUANT_ROWS = [r for r in T.Q8_INSTANTIATIONS if r.kind == "rows"]
QR_LDS_FLOATS = 16380   # csrc_q8/quant_rows_s8.hpp


def _last(x, tile):
    """The width of the last tile along a dimension of x."""
    return x - (math.ceil(x / tile) - 1) * tile


@pytest.mark.parametrize("row", GEMM_ROWS, ids=lambda r: r.symbol)
def test_every_case_reaches_its_row(row):
    cases = row.cases(CUS)
    assert cases and len(set(cases)) == len(cases), row.symbol
    for c in cases:
        text, _ = R.plan_text(c.rows, c.out, c.in_, *T.layout_of(c), row.bias, row.relu, CUS)
        assert text.endswith(f"then {row.symbol}, {math.ceil(c.rows / row.tile) * math.ceil(c.out / row.tile)} workgroups"), (row.symbol, c, text)
        assert R.big_tile(c.rows, c.out, CUS) == (row.tile == 256), c
    assert len(GEMM_ROWS) == 16


@pytest.mark.parametrize("row", GEMM_ROWS, ids=lambda r: r.symbol)
def test_the_gemm_rows_cover_k_depths_and_tails_thin_tiles_layouts_and_grids(row):
    cases = row.cases(CUS)
    tile = row.tile
    ks = {c.in_ for c in cases}
    if not row.edge:
        want = set(T.KS_Q8 if tile == 128 else T.KS_256)
        assert want <= ks, (row.symbol, sorted(want - ks))
        assert all(c.rows % tile == 0 and c.out % tile == 0 and c.ldy_pad % 4 == 0 and c.off_y % 4 == 0 for c in cases), row.symbol
        assert any(c[3:] == (0, 0, 0, 0) for c in cases), (row.symbol, "no dense case")
        assert {0, 4} <= {c.ldy_pad for c in cases}, row.symbol
    assert {1, 2, 3, 4} <= {math.ceil(k / 256) for k in ks}, (row.symbol, sorted(ks))   # trips of the tile's K loop
    if tile == 128:   # the last pair of slices: the odd one empty, one byte, full
        assert {128, 129, 256} <= {k - 256 * (math.ceil(k / 256) - 1) for k in ks}, row.symbol
        assert any(k % 4 for k in ks) and any(k % 16 and not k % 4 for k in ks) and any(k % 64 and not k % 16 for k in ks), row.symbol
    if row.edge:
        for name, thin in (("rows", {_last(c.rows, tile) for c in cases if c.rows > tile}), ("out", {_last(c.out, tile) for c in cases if c.out > tile})):
            assert set(T.THIN) <= thin, (row.symbol, name, sorted(set(T.THIN) - thin))
        assert {1, 2, 3} <= {c.ldy_pad for c in cases}, row.symbol
        assert {0, 1} <= {c.off_y for c in cases}, row.symbol
        # guarded on whole tiles: by an odd ldy alone, the base aligned
        assert any(c.rows % tile == 0 and c.out % tile == 0 and c.ldy_pad % 2 == 1 and c.off_y % 4 == 0 for c in cases), row.symbol
    if tile == 128:
        grids = {(math.ceil(c.rows / tile), math.ceil(c.out / tile)) for c in cases}
        assert any(a * b > 8 and (a * b) % 8 for a, b in grids), (row.symbol, sorted(grids))
        assert any(a == 1 and b > 8 for a, b in grids) and any(b == 1 and a > 8 for a, b in grids), (row.symbol, sorted(grids))


def test_the_quantiser_rows_cover_both_forms_on_both_paths_and_the_lds_cap():
    assert [r.symbol for r in QUANT_ROWS] == ["quantize_rows_s8_kernel<false>", "quantize_rows_s8_kernel<true>"]
    narrow, wide = (r.cases(CUS) for r in QUANT_ROWS)
    assert sorted(narrow + wide) == sorted(T.quant_cases())
    for cases, is_wide in ((narrow, False), (wide, True)):
        assert all((cols >= 1024) == is_wide for _, cols, _ in cases)
        assert {vec for _, _, vec in cases} == {True, False}
        assert {1, 2, 5} <= {rows for rows, _, _ in cases}
    assert {3, 4, 5} <= {cols for _, cols, vec in narrow if vec}
    # (a one-row tensor's leading dimension is its width: only a multiple of 4 columns keeps it on the vector path)
    assert all(cols % 4 == 0 for rows, cols, _ in narrow + wide if rows == 1)
    # columns behind the last float4 of a vector-path row, inside and beyond what the wide form keeps in LDS
    tails = [cols for _, cols, vec in wide if vec and cols % 4]
    assert any(c < QR_LDS_FLOATS for c in tails) and any(c > QR_LDS_FLOATS + 4 for c in tails), tails
    for vec in (True, False):
        assert {16379, 16380, 16381, 16383, 16384} <= {cols for _, cols, v in wide if v == vec}
    # ... and through the layer: both paths, a float4 tail, both sides of the cap
    layer = T.WIDE_LAYER
    assert all(s[2] >= 1024 for s, _ in layer) and {v for _, v in layer} == {True, False}
    assert any(v and s[2] % 4 and s[2] > QR_LDS_FLOATS for s, v in layer) and any(v and s[2] % 4 and s[2] < QR_LDS_FLOATS for s, v in layer)
    assert any(not v and s[2] > QR_LDS_FLOATS for s, v in layer)


@built_lib.needs_library
def test_the_librarys_plan_says_the_same_of_every_case():
    """mmh_q8_linear_plan (host arithmetic in libmmult_hip_q8.so) on every case's leading dimensions and base residues."""
    if not built_lib.library_loads():
        pytest.skip("libmmult_hip_q8.so (or the HIP runtime it links) is not loadable here")
    from how_to_optimize_gemm_amd import q8
    for row in GEMM_ROWS:
        for c in row.cases(CUS):
            args = (c.rows, c.out, c.in_, *T.layout_of(c))
            assert q8.qlinear_plan(*args, row.bias, "relu" if row.relu else None, CUS) == R.plan_text(*args, row.bias, row.relu, CUS), (row.symbol, c)
