"""The int8 linear layer on the GPU (libmmult_hip_q8.so, how_to_optimize_gemm_amd.q8), bit for bit against tests/qlinear_ref.py.

Q8_INSTANTIATIONS holds one row per kernel symbol of the library (tests/test_q8_kernel_census.py holds the table to the
library, both ways): the GEMM's sixteen instantiations -- tile x guarded x bias x ReLU --, the row quantiser's two forms and
the weight image's kernel.  A GEMM row runs every shape of its (tile, guarded) class; mmh_q8_last_launch must name the row's
symbol.  x has a padded leading dimension, y a padded one poisoned with NaN that must survive.

The 256x256 shapes are chosen by csrc/igemm_plan.hpp's i8_big_tile with the test device's CU count (qlinear_ref.big_tile):
the smallest multiple-of-256 shape that takes the big tile, a ragged neighbour, and the smallest shapes whose last tiles are
THIN wide.

Every GEMM row also has a case table (Row.cases; tests/test_q8_coverage.py holds the classes it promises, on the CPU): one
test id per (tile, guarded, case) runs the class's four epilogues on inputs whose every 128-byte slice of k moves the sums.
The tile's K loop requests slice kt + 2 while it works on slice kt, so only an inner dimension beyond 256 refills an LDS
buffer with data inside the loop: KS_Q8 / KS_256 reach one to four trips and every tail of the last pair of slices."""
import collections
import functools
import math

import numpy as np
import pytest

import qlinear_ref as R
from bitcmp import first_difference, same_bits
from gpu_operands import _padded, cus_fixture, handle_fixture
from qlinear_ref import IN_256, shapes_256, thin_256   # (shared with tests/q8_fuzz.py)

pytestmark = pytest.mark.gpu

amm = handle_fixture()        # asked for the device's CU count only
cus = cus_fixture("amm")


class Row(collections.namedtuple("Row", "symbol kind tile edge bias relu")):
    __slots__ = ()

    def cases(self, cu_count):
        """The row's cases (a GEMM row: those of its (tile, guarded) class; a quantiser row: (rows, cols, vector path))."""
        if self.kind == "gemm":
            return gemm_cases(self.tile, self.edge, cu_count)
        wide = self.symbol.endswith("<true>")
        return [c for c in quant_cases() if (c[1] >= 1024) == wide] if self.kind == "rows" else []


_B = {False: "false", True: "true"}
Q8_INSTANTIATIONS = [Row(f"qlinear_s8_kernel<{t},{t},{t // 32},{_B[e]},{_B[b]},{_B[r]}>", "gemm", t, e, b, r)
                     for t in (128, 256) for e in (False, True) for b in (False, True) for r in (False, True)]
Q8_INSTANTIATIONS += [Row("quantize_rows_s8_kernel<false>", "rows", 0, False, False, False),
                      Row("quantize_rows_s8_kernel<true>", "rows", 0, False, False, False),
                      Row("prepare_weight_s8_kernel", "weight", 0, False, False, False)]

SHAPES_128 = {False: [(128, 128, 128), (128, 128, 64)], True: [(129, 130, 131), (5, 3, 7), (1, 1, 1)]}
# stand-alone quantiser / weight shapes (rows x cols).  Wave per row: 1 - 5 and 1023 columns (five rows: the last one alone in
# a second workgroup); workgroup per row from 1024 on, with and without columns behind the last float4, and on both sides of
# the 16380 floats the workgroup form keeps in LDS (a longer row's rest is read again)
ALONE = [(3, 1), (7, 1023), (4, 1024), (2, 5000), (2, 16392)]
ALONE += [(5, 3), (1, 4), (2, 5)]
ALONE += [(2, 1025), (5, 1027), (2, 5003), (5, 16379), (1, 16380), (2, 16381), (5, 16383), (1, 16384), (2, 16393), (5, 20001)]

# ---- the GEMM rows' case table ----------------------------------------------------------------------------------------------
# a slice is 128 bytes and a loop trip two slices: trips 1 .. 4, the odd slice of the last pair empty, one byte, full; tails
# that are no multiple of 64, 16 or 4
KS_Q8 = (1, 3, 4, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 385, 512, 513, 641, 777)
KS_256 = (129, 257, 513, 777)
KS_256_EDGE = (192, 129, 257, 385, 513, 641, 777)
THIN = (1, 3, 4, 5, 15, 16, 17)   # last tiles: y's stores go in 4 columns, the transposer in 16 rows

# (ldx_pad, ldy_pad, off_x, off_y): floats behind a row of x / y, floats between the allocation and the base
Case = collections.namedtuple("Case", "rows out in_ ldx_pad ldy_pad off_x off_y")
WHOLE_LAYOUT, EDGE_LAYOUT = (4, 4, 4, 4), (3, 1, 1, 1)
# whole tiles need ldy % 4 == 0 and a 16-byte aligned y; x only decides the quantiser's path.  The first is fully dense
WHOLE_LAYOUTS = ((0, 0, 0, 0), (4, 4, 4, 4), (3, 0, 1, 4), (1, 4, 2, 0), (0, 4, 0, 4))
GEMM_CLASSES = [(t, e) for t in (128, 256) for e in (False, True)]


def gemm_cases(tile, edge, cu_count):
    """The Cases of a (tile, guarded) class; the same number on every device."""
    cases = []
    if tile == 128 and not edge:
        cases += [Case(*s, *WHOLE_LAYOUT) for s in SHAPES_128[False]]
        cases += [Case(128, 128, k, *WHOLE_LAYOUTS[i % 5]) for i, k in enumerate(KS_Q8)]
        # grids: 9 tiles (no multiple of the 8 XCDs), 1 x 17, 17 x 1
        cases += [Case(384, 384, 64, *WHOLE_LAYOUT), Case(128, 2176, 64, *WHOLE_LAYOUTS[0]), Case(2176, 128, 64, *WHOLE_LAYOUTS[2])]
    elif tile == 128:
        cases += [Case(*s, *EDGE_LAYOUT) for s in SHAPES_128[True]]
        cases += [Case(128 + THIN[i % 7], 128 + THIN[(i + 3) % 7], k, (3, 0, 4, 1)[i % 4], (1, 2, 3)[i % 3], (1, 0, 4, 2)[i % 4], i % 2)
                  for i, k in enumerate(KS_Q8)]
        cases += [Case(128, 128, 64, 4, 1, 4, 0),              # guarded on whole tiles by an odd ldy alone, the base aligned
                  Case(637, 379, 65, *EDGE_LAYOUT),            # 5 x 3 tiles
                  Case(100, 2177, 64, 0, 2, 0, 1), Case(2177, 100, 64, 4, 3, 4, 0)]   # 1 x 18, 18 x 1
    elif not edge:
        m, n, _ = shapes_256(cu_count)[0]
        cases += [Case(m, n, IN_256, *WHOLE_LAYOUT)]
        cases += [Case(m, n, k, *WHOLE_LAYOUTS[i]) for i, k in enumerate(KS_256)]
    else:
        (m, n, _), ragged = shapes_256(cu_count)
        cases += [Case(*ragged, *EDGE_LAYOUT)]
        cases += [Case(*thin_256(THIN[i], THIN[(i + 3) % 7], cu_count), k, (3, 0, 4, 1)[i % 4], (1, 2, 3)[i % 3], (1, 0, 4, 2)[i % 4], i % 2)
                  for i, k in enumerate(KS_256_EDGE)]
        cases += [Case(m, n, IN_256, 4, 1, 4, 0)]
    return cases


def quant_cases():
    """(rows, cols, vector path) of the stand-alone row quantiser: every shape of ALONE on both paths."""
    return [(rows, cols, aligned) for aligned in (True, False) for rows, cols in ALONE]


def layout_of(c):
    """(ldx, ldy, x's base modulo 16, y's) of a Case."""
    return c.in_ + c.ldx_pad if c.in_ else 4, c.out + c.ldy_pad, 4 * c.off_x % 16, 4 * c.off_y % 16


def every_slice_matters(qx, qw):
    """Zeroing any one 128-byte slice of qx changes at least 99 % of the sums (of the first 128 x 128 of them)."""
    qx, qw = qx[:128], qw[:128]
    for k0 in range(0, qx.shape[1], 128):
        unchanged = float((R.int_sums(qx[:, k0:k0 + 128], qw[:, k0:k0 + 128]) == 0).mean())
        assert unchanged <= 0.01, (qx.shape, qw.shape, k0, unchanged)


@functools.lru_cache(maxsize=1)
def deep_problem(rows, out, in_):
    """problem()'s distributions; the last column of every row of x and of w is plus or minus that row's maximum (a dropped
    last byte moves every sum by 127^2).  Asserts on the host that every slice matters."""
    rng = np.random.default_rng(rows * 7 + out * 3 + in_ + 1)
    x = (rng.standard_normal((rows, in_)) * 3).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, (out, in_)).astype(np.float32)
    bias = rng.uniform(-4, 4, out).astype(np.float32)
    for v in (x, w):
        v[:, -1] = np.abs(v).max(axis=1) * rng.choice(np.array([-1, 1], np.float32), v.shape[0])
    qx, _, rx = R.quantize_rows_ref(x)
    qw, _, rw = R.quantize_rows_ref(w)
    every_slice_matters(qx, qw)
    return x, w, bias, (R.int_sums(qx, qw), rx, rw)


@functools.lru_cache(maxsize=4)
def problem(rows, out, in_):
    """Inputs of a shape and the parts of its reference every epilogue shares."""
    rng = np.random.default_rng(rows * 7 + out * 3 + in_)
    x = (rng.standard_normal((rows, in_)) * 3).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, (out, in_)).astype(np.float32)
    bias = rng.uniform(-4, 4, out).astype(np.float32)
    return x, w, bias, parts(x, w)


def parts(x, w):
    qx, _, rx = R.quantize_rows_ref(x)
    qw, _, rw = R.quantize_rows_ref(w)
    return R.int_sums(qx, qw), rx, rw


_weights = {}


def weight_of(key, w):
    """One prepared weight per shape (the epilogue variants of a shape share it)."""
    import torch
    from how_to_optimize_gemm_amd import q8
    if key not in _weights:
        _weights.clear()
        _weights[key] = q8.QWeight(torch.from_numpy(w).cuda())
    return _weights[key]


def _layout(guarded, off=None):
    """EDGE_LAYOUT -- odd leading dimensions, bases 4 bytes past 16-byte alignment -- or WHOLE_LAYOUT -- leading dimensions
    that are multiples of 4 floats past the row, 16-byte aligned bases; `off`: both bases that many floats in instead."""
    lay = EDGE_LAYOUT if guarded else WHOLE_LAYOUT
    return lay if off is None else (lay[0], lay[1], off, off)


def run(qw, x, bias, relu, ldx_pad, ldy_pad, off_x, off_y, bias_off=0):
    """qlinear on NaN-padded operands: ldx_pad / ldy_pad floats behind every row of x / y, the bases off_x / off_y floats
    into their allocations, the bias bias_off floats into its own.  Returns (y's window, nothing outside it was written, the
    launch text)."""
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, in_ = x.shape
    out = qw.out_features
    ldx = in_ + ldx_pad if in_ else 4
    ldy = out + ldy_pad
    _, xv = _padded(rows, in_, ldx, off_x, x)
    yflat, yv = _padded(rows, out, ldy, off_y)
    db = None
    if bias is not None:
        db = torch.full((bias_off + out + 4,), float("nan"), device="cuda")[bias_off:bias_off + out]
        db.copy_(torch.from_numpy(bias))
    q8.qlinear(xv[:, :in_], qw, db, "relu" if relu else None, out=yv[:, :out])
    launched = q8.last_launch()
    torch.cuda.synchronize()
    untouched = bool(torch.isnan(yv[:, out:]).all()) and bool(torch.isnan(yflat[:off_y]).all()) and \
        bool(torch.isnan(yflat[off_y + rows * ldy:]).all())
    return yv[:, :out].cpu().numpy(), untouched, launched


def check(shape, bias, relu, guarded, symbol, cu_count, off=None):
    rows, out, in_ = shape
    x, w, b, (acc, rx, rw) = problem(*shape)
    got, untouched, launched = run(weight_of(shape, w), x, b if bias else None, relu, *_layout(guarded, off))
    want = R.epilogue_ref(acc, rx, rw, b if bias else None, relu)
    assert symbol in launched, (shape, symbol, launched)
    assert same_bits(got, want), (shape, launched, first_difference(got, want))
    assert untouched, (shape, "wrote outside y's window")
    return launched


@pytest.mark.parametrize("row", [r for r in Q8_INSTANTIATIONS if r.kind == "gemm"], ids=lambda r: r.symbol)
def test_every_instantiation_is_reached_and_is_the_contract(row, cus):
    if row.tile == 128:
        shapes = SHAPES_128[row.edge]
    else:
        shapes = [shapes_256(cus)[1 if row.edge else 0]]
    for shape in shapes:
        launched = check(shape, row.bias, row.relu, row.edge, row.symbol, cus)
        # ... and the launch is what mmh_q8_linear_plan says for the call
        rows, out, in_ = shape
        off = 4 if row.edge else 0
        text, _ = R.plan_text(rows, out, in_, in_ + (3 if row.edge else 4), out + (1 if row.edge else 4), off, off, row.bias, row.relu, cus)
        assert launched == text


def check_case(c, x, w, b, acc, rx, rw, qw, row, cu_count, bias_off=0):
    """One Case in one epilogue: the launch is the row's symbol and the plan's text, y is the contract, nothing else is written."""
    got, untouched, launched = run(qw, x, b if row.bias else None, row.relu, *c[3:], bias_off=bias_off)
    want = R.epilogue_ref(acc, rx, rw, b if row.bias else None, row.relu)
    text, _ = R.plan_text(c.rows, c.out, c.in_, *layout_of(c), row.bias, row.relu, cu_count)
    assert row.symbol in launched and launched == text, (c, row.symbol, launched, text)
    assert same_bits(got, want), (c, launched, first_difference(got, want))
    assert untouched, (c, launched, "wrote outside y's window")


def rows_of(tile, edge):
    return [r for r in Q8_INSTANTIATIONS if r.kind == "gemm" and (r.tile, r.edge) == (tile, edge)]


@pytest.mark.parametrize("tile,edge,index", [(t, e, i) for t, e in GEMM_CLASSES for i in range(len(gemm_cases(t, e, 256)))],
                         ids=lambda v: {False: "whole", True: "guarded"}[v] if isinstance(v, bool) else str(v))
def test_every_case_of_the_table_is_the_contract_in_its_four_epilogues(tile, edge, index, cus):
    """K depth and tails, thin last tiles, grids, leading dimensions and bases (gemm_cases) on deep_problem's inputs."""
    import torch
    from how_to_optimize_gemm_amd import q8
    cases = gemm_cases(tile, edge, cus)
    assert len(cases) == len(gemm_cases(tile, edge, 256))
    c = cases[index]
    x, w, b, (acc, rx, rw) = deep_problem(c.rows, c.out, c.in_)
    qw = q8.QWeight(torch.from_numpy(w).cuda())
    for row in rows_of(tile, edge):
        check_case(c, x, w, b, acc, rx, rw, qw, row, cus)
    qw.close()


@pytest.mark.parametrize("edge", [False, True], ids=["whole", "guarded"])
def test_a_bias_four_bytes_past_alignment(edge, cus):
    """The header allows any 4-byte aligned bias: a unit-stride view that starts 4 bytes past a 16-byte boundary."""
    import torch
    from how_to_optimize_gemm_amd import q8
    c = Case(128, 128, 257, *WHOLE_LAYOUT) if not edge else Case(133, 143, 257, *EDGE_LAYOUT)
    x, w, b, (acc, rx, rw) = deep_problem(c.rows, c.out, c.in_)
    qw = q8.QWeight(torch.from_numpy(w).cuda())
    for row in rows_of(128, edge):
        if row.bias:
            check_case(c, x, w, b, acc, rx, rw, qw, row, cus, bias_off=1)
    qw.close()


# (rows, out, in), the quantiser's path: the workgroup-per-row quantiser feeding the GEMM -- at its first width, with columns
# behind the last float4, and beyond what it keeps in LDS (whole tiles on the vector path; the scalar path, 79 loop trips)
WIDE_LAYER = [((5, 3, 1024), True), ((5, 3, 1024), False), ((130, 70, 1027), True), ((130, 70, 1027), False),
              ((128, 128, 16393), True), ((129, 130, 20001), False)]


@pytest.mark.parametrize("shape,vector", WIDE_LAYER, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("scalar", "vector")[v])
def test_the_wide_row_quantiser_feeds_the_gemm(shape, vector, cus):
    """Ordinary random data through quantize_rows_s8_kernel<true> and the GEMM; in the long shapes one row of x (and one channel
    of w) has NaN, +inf, -inf, -0.0 and its maximum in columns the quantiser does not keep in LDS."""
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, out, in_ = shape
    rng = np.random.default_rng(in_ + rows)
    x = (rng.standard_normal((rows, in_)) * 3).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, (out, in_)).astype(np.float32)
    b = rng.uniform(-4, 4, out).astype(np.float32)
    if in_ > 16384:
        for v, r, top in ((x, rows - 2, 40.0), (w, 1, -2.0)):
            v[r, 16380:16384] = [np.nan, np.inf, -np.inf, -0.0]
            v[r, in_ - 1] = top
            assert np.abs(v[r, :16380]).max() < abs(top)
    c = Case(rows, out, in_, -in_ % 4, 4, 4, 4) if vector else Case(rows, out, in_, *EDGE_LAYOUT)
    qw = q8.QWeight(torch.from_numpy(w).cuda())
    for bias, relu in ((None, False), (b, True)):
        got, untouched, launched = run(qw, x, bias, relu, *c[3:])
        text, _ = R.plan_text(rows, out, in_, *layout_of(c), bias is not None, relu, cus)
        assert launched == text and launched.startswith(f"quantize_rows_s8_kernel<true> ({'vector' if vector else 'scalar'} path)"), launched
        want = R.qlinear_ref(x, w, bias, relu)
        assert same_bits(got, want) and untouched, (launched, first_difference(got, want))
    qw.close()


def test_operands_four_bytes_past_alignment_take_the_guarded_tile_and_the_scalar_quantiser(cus):
    """A whole-tile shape with multiple-of-4 leading dimensions whose x and y start 4 bytes past a 16-byte boundary."""
    launched = check((128, 128, 64), True, True, False, "qlinear_s8_kernel<128,128,4,true,true,true>", cus, off=1)
    assert launched.startswith("quantize_rows_s8_kernel<false> (scalar path)")
    launched = check((128, 128, 64), True, True, False, "qlinear_s8_kernel<128,128,4,false,true,true>", cus, off=4)
    assert launched.startswith("quantize_rows_s8_kernel<false> (vector path)")


def test_an_empty_inner_dimension_is_the_formula_on_zero_sums(cus):
    import torch
    from how_to_optimize_gemm_amd import q8
    w, x = np.zeros((3, 0), np.float32), np.zeros((4, 0), np.float32)
    bias = np.array([1.5, -0.0, -2.0], np.float32)
    qw = q8.QWeight(_padded(3, 0, 4, 4)[1][:, :0])   # (a (3, 0) window with a row stride: numpy's own has stride 0)
    for b, relu in ((None, False), (bias, False), (bias, True)):
        got, untouched, _ = run(qw, x, b, relu, *EDGE_LAYOUT)
        want = R.qlinear_ref(x, w, b, relu)
        assert same_bits(got, want) and untouched, (relu, got, want)
    assert same_bits(R.qlinear_ref(x, w, bias, True), np.tile(np.array([1.5, 0.0, 0.0], np.float32), (4, 1)))


FUZZ_EMPTY_IN = (53, 271, 0)   # (rows, out, in) of the fuzz case that found it (tests/q8_fuzz.py: cases(64, 2026, 256)[9])


def test_the_row_quantiser_takes_an_empty_inner_dimension_and_feeds_the_int8_output(cus):
    """A (rows, 0) tensor has no bytes and torch gives it the address NULL: mmh_q8_quantize_rows took the NULL dQ for an argument
    error, so quantize_rows, quantize and an int8-output qlinear on fp32 rows raised where in == 0.  Every scale is 1, nothing
    of the window is written, and the layer is the requantised bias."""
    import torch
    import qchain_ref as Q
    from how_to_optimize_gemm_amd import q8
    rows, out, _ = FUZZ_EMPTY_IN
    x = _padded(rows, 0, 4, 4)[1][:, :0]
    window = torch.full((rows, 8), 0x55, dtype=torch.int8, device="cuda")
    q, s, r = q8.quantize_rows(x, out=window[:, :0])
    launched = q8.last_launch()
    torch.cuda.synchronize()
    assert launched.startswith("quantize_rows_s8_kernel<false>") and launched.endswith(f"{(rows + 3) // 4} workgroups"), launched
    assert tuple(q.shape) == (rows, 0) and bool((window == 0x55).all())
    ones = np.ones(rows, np.float32)
    assert same_bits(s.cpu().numpy(), ones) and same_bits(r.cpu().numpy(), ones)
    xq = q8.quantize(x)
    assert (xq.rows, xq.cols) == (rows, 0) and same_bits(xq.inv_scale.cpu().numpy(), ones)
    bias = np.random.default_rng(53).uniform(-4, 4, out).astype(np.float32)
    bias[:4] = [0.25, -1.25, 63.75, -100.0]   # ties at the scale 2, and a value that clamps
    qw = q8.QWeight(_padded(out, 0, 4, 4)[1][:, :0])
    for relu in (False, True):
        got = q8.qlinear(x, qw, torch.from_numpy(bias).cuda(), "relu" if relu else None, out_scale=2.0)
        torch.cuda.synchronize()
        want = Q.requant_ref(R.qlinear_ref(np.zeros((rows, 0), np.float32), np.zeros((out, 0), np.float32), bias, relu), np.full(rows, 2.0, np.float32))
        assert np.array_equal(got.q.cpu().numpy(), want) and same_bits(got.inv_scale.cpu().numpy(), np.full(rows, 0.5, np.float32)), relu
        assert (want[0, :4] == ([0, 0, 127, 0] if relu else [0, -2, 127, -127])).all()
    qw.close()


def test_large_sums_round_to_nearest_even(cus):
    """(64, 64, 2048), every |element| its row's maximum: every q is +-127, |acc| up to 127^2 * 2048 > 2^24."""
    import torch
    from how_to_optimize_gemm_amd import q8
    rng = np.random.default_rng(11)
    x = np.where(rng.random((64, 2048)) < 0.05, -1.5, 1.5).astype(np.float32) * rng.uniform(0.5, 2, (64, 1)).astype(np.float32)
    w = np.where(rng.random((64, 2048)) < 0.05, -0.25, 0.25).astype(np.float32) * rng.uniform(0.5, 2, (64, 1)).astype(np.float32)
    x[0], w[0] = 1.5, 0.25
    acc, rx, rw = parts(x, w)
    assert acc[0, 0] == 127 * 127 * 2048 and (np.abs(acc) > 1 << 24).sum() > 1000
    check_large(x, w, acc, rx, rw)
    # 127^2 times an even count is even, and below 2^25 every even integer is a float32: the sums above convert exactly.  One
    # element per row of x at 2 / 127 of the maximum (q = 2: 127^2 times an odd count, plus or minus 254) makes them odd: now float32(acc) has to round
    x[:, 5] *= np.float32(2.0 / 127.0)
    acc, rx, rw = parts(x, w)
    assert (np.abs(acc) > 1 << 24).sum() > 1000 and (acc.astype(np.float32).astype(np.int64) != acc).sum() > 1000
    check_large(x, w, acc, rx, rw)
    # the same below -2^24: every other channel of w negated
    w[::2] = -w[::2]
    acc, rx, rw = parts(x, w)
    low = acc < -(1 << 24)
    assert low.sum() > 1000 and (acc.astype(np.float32).astype(np.int64) != acc)[low].sum() > 1000
    check_large(x, w, acc, rx, rw)


def test_special_values_in_the_bias(cus):
    """+inf, -inf, NaN, -0.0 and +0.0 as biases of non-zero sums, with and without ReLU (NaN stays, -inf and -0.0 give +0)."""
    import torch
    from how_to_optimize_gemm_amd import q8
    rng = np.random.default_rng(17)
    x = rng.standard_normal((9, 40)).astype(np.float32)
    w = rng.uniform(-1, 1, (11, 40)).astype(np.float32)
    bias = rng.uniform(-1, 1, 11).astype(np.float32)
    bias[[0, 2, 4, 6, 8]] = [np.inf, -np.inf, np.nan, -0.0, 0.0]
    assert np.count_nonzero(parts(x, w)[0]) > 90
    qw = q8.QWeight(torch.from_numpy(w).cuda())
    for relu in (False, True):
        got, untouched, launched = run(qw, x, bias, relu, *EDGE_LAYOUT)
        want = R.qlinear_ref(x, w, bias, relu)
        assert same_bits(got, want) and untouched, (launched, first_difference(got, want))
        assert np.isnan(want[:, 4]).all() and (want[:, 2] == (0 if relu else -np.inf)).all()


def check_large(x, w, acc, rx, rw):
    import torch
    from how_to_optimize_gemm_amd import q8
    got, untouched, launched = run(q8.QWeight(torch.from_numpy(w).cuda()), x, None, False, *WHOLE_LAYOUT)
    want = R.epilogue_ref(acc, rx, rw)
    assert same_bits(got, want) and untouched, (launched, first_difference(got, want))


def test_special_values_as_activation_rows_and_as_weight_channels(cus):
    import torch
    from how_to_optimize_gemm_amd import q8
    rng = np.random.default_rng(5)
    special = np.stack([r for _, r, _, _ in R.special_rows(40, rng)])
    plain = rng.uniform(-1, 1, (6, 40)).astype(np.float32)
    bias = rng.uniform(-1, 1, 11).astype(np.float32)
    both = np.concatenate([special, plain])
    for x, w in ((both, both), (plain, both), (both, plain)):
        b = bias[:w.shape[0]]
        qw = q8.QWeight(torch.from_numpy(w).cuda())
        for relu in (False, True):
            got, untouched, launched = run(qw, x, b, relu, *EDGE_LAYOUT)
            want = R.qlinear_ref(x, w, b, relu)
            assert same_bits(got, want) and untouched, (launched, first_difference(got, want))


def _quant_input(rows, cols, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, cols)) * 2).astype(np.float32)
    if cols >= 9:
        x[0, :9] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-38, -1e-38, 5.0, -5.0]
    if cols > 9:   # the same at the end of the row, where a long row is not kept in LDS, with the row's maximum in the last column
        x[0, -9:] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-38, -1e-38, 50.0, -50.0]
    if rows > 1:
        x[1] = 0.0
    if cols > 9 and rows > 2:   # a later row: ordinary data, the maximum in the last column
        x[rows - 1, -1] = 100.0
    return x


@pytest.mark.parametrize("rows,cols", ALONE)
@pytest.mark.parametrize("aligned", [True, False], ids=["vector", "scalar"])
def test_the_row_quantiser_alone(rows, cols, aligned):
    """q, scale, inv_scale and the zeroed pad bytes; x with a padded leading dimension, q in a poisoned buffer whose bytes
    beyond the pad must survive."""
    import torch
    from how_to_optimize_gemm_amd import q8
    x = _quant_input(rows, cols, rows + cols)
    ldx = ((cols + 3) & ~3) + 4 if aligned else cols + 3
    _, xv = _padded(rows, cols, ldx, 4 if aligned else 1, x)
    pitch = (cols + 15) & ~15
    ldq = pitch + 32 if aligned else cols + 5          # (the second: fewer bytes behind the row than the pad asks for)
    qflat = torch.full((16 + rows * ldq + 16,), 0x55, dtype=torch.int8, device="cuda")
    off = 16 if aligned else 17
    qv = qflat[off:off + rows * ldq].view(rows, ldq)
    q, s, r = q8.quantize_rows(xv[:, :cols], out=qv[:, :cols])
    launched = q8.last_launch()
    torch.cuda.synchronize()
    # (a one-row tensor has no row stride: the binding passes its width as the leading dimension, and nothing lies behind the row)
    vector = aligned and (rows > 1 or cols % 4 == 0)
    assert launched == f"quantize_rows_s8_kernel<{_B[cols >= 1024]}> ({'vector' if vector else 'scalar'} path), " \
                       f"{rows if cols >= 1024 else (rows + 3) // 4} workgroups"
    wq, ws, wr = R.quantize_rows_ref(x)
    got = qv.cpu().numpy()
    pad_to = min(ldq, pitch) if rows > 1 else cols
    assert np.array_equal(got[:, :cols], wq) and not got[:, cols:pad_to].any() and (got[:, pad_to:] == 0x55).all()
    flat = qflat.cpu().numpy()
    assert (flat[:off] == 0x55).all() and (flat[off + rows * ldq:] == 0x55).all()
    assert same_bits(s.cpu().numpy(), ws) and same_bits(r.cpu().numpy(), wr)
    # the default output: rows of `pitch` bytes
    q2, s2, r2 = q8.quantize_rows(xv[:, :cols])
    assert np.array_equal(q2.cpu().numpy(), wq) and same_bits(s2.cpu().numpy(), ws) and same_bits(r2.cpu().numpy(), wr)


# (the image is in_ x out rounded up to 16 bytes: shapes whose image stays below 4 MB)
@pytest.mark.parametrize("out,in_", [s for s in ALONE + [(130, 70)] if s[1] * ((s[0] + 15) & ~15) < 4 << 20])
@pytest.mark.parametrize("aligned", [True, False], ids=["vector", "scalar"])
def test_the_weight_image_alone(out, in_, aligned):
    """QWeight: the image is the per-channel quantisation transposed, pad columns 0; scale and inv_scale per channel."""
    import torch
    from how_to_optimize_gemm_amd import q8
    w = _quant_input(out, in_, out * 3 + in_)
    ldw = ((in_ + 3) & ~3) + 4 if aligned else in_ + 3
    _, wv = _padded(out, in_, ldw, 4 if aligned else 1, w)
    qw = q8.QWeight(wv[:, :in_])
    img, s, r = qw.q.cpu().numpy(), qw.scale.cpu().numpy(), qw.inv_scale.cpu().numpy()
    wq, ws, wr = R.quantize_rows_ref(w)
    assert qw.pitch == (out + 15) & ~15 and img.shape == (in_, qw.pitch) and img.dtype == np.int8
    assert np.array_equal(img[:, :out], wq.T) and not img[:, out:].any()
    assert same_bits(s, ws) and same_bits(r, wr)
    qw.close()


def test_one_weight_serves_calls_of_different_rows_and_grows_its_scratch(cus):
    import torch
    from how_to_optimize_gemm_amd import q8
    rng = np.random.default_rng(3)
    w = rng.uniform(-1, 1, (70, 50)).astype(np.float32)
    bias = rng.uniform(-1, 1, 70).astype(np.float32)
    qw = q8.QWeight(torch.from_numpy(w).cuda())
    qw.reserve(16)
    for rows in (16, 3, 200):   # (200: past what was reserved, eagerly)
        x = rng.standard_normal((rows, 50)).astype(np.float32)
        got, untouched, launched = run(qw, x, bias, True, *EDGE_LAYOUT)
        want = R.qlinear_ref(x, w, bias, True)
        assert same_bits(got, want) and untouched, (rows, launched, first_difference(got, want))


def _side_stream():
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    return side


def _capture(side, body):
    import torch
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            body()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def test_growth_under_capture_is_refused_and_growth_after_it_retires():
    """A captured call that would have to grow the weight's scratch is MMH_ERR_UNSUPPORTED with y untouched and the capture
    goes on; once a captured call has used the scratch, eager growth keeps the old buffer for the graph."""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    rng = np.random.default_rng(9)
    w = rng.uniform(-1, 1, (40, 36)).astype(np.float32)
    qw = q8.QWeight(torch.from_numpy(w).cuda())
    xs, xl = torch.zeros((8, 36), device="cuda"), torch.zeros((64, 36), device="cuda")
    ys, yl = torch.full((8, 40), float("nan"), device="cuda"), torch.full((64, 40), float("nan"), device="cuda")
    side = _side_stream()
    with torch.cuda.stream(side):
        q8.qlinear(xs, qw, out=ys)   # the eager warm-up: sizes the scratch for 8 rows
    side.synchronize()
    seen = []

    def body():
        q8.qlinear(xs, qw, out=ys)
        # (no `pytest.raises(...) as e` here: its ExceptionInfo and this frame would form a cycle that keeps _capture's graph
        # alive until some later garbage collection -- possibly inside another test's capture, where destroying a
        # torch.cuda.CUDAGraph is not safe on ROCm)
        try:
            q8.qlinear(xl, qw, out=yl)
        except H.MMultError as err:
            seen.append(err.status)

    graph = _capture(side, body)
    assert seen == [H.ERR_UNSUPPORTED]
    a = rng.standard_normal((8, 36)).astype(np.float32)
    xs.copy_(torch.from_numpy(a))
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(ys.cpu().numpy(), R.qlinear_ref(a, w)) and bool(torch.isnan(yl).all())
    # eager growth after the capture: exact, and the graph still replays on the buffer it points at
    b = rng.standard_normal((64, 36)).astype(np.float32)
    xl.copy_(torch.from_numpy(b))
    q8.qlinear(xl, qw, out=yl)
    torch.cuda.synchronize()
    assert same_bits(yl.cpu().numpy(), R.qlinear_ref(b, w))
    a = rng.standard_normal((8, 36)).astype(np.float32)
    xs.copy_(torch.from_numpy(a))
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(ys.cpu().numpy(), R.qlinear_ref(a, w))
    del graph


def test_a_captured_call_replays_the_contract_on_new_inputs():
    """One qlinear captured after an eager warm-up on the capture stream (a single-stream chain: the row quantiser, then the
    GEMM), replayed three times on new x: each replay is the eager result and the reference, bit for bit."""
    import torch
    from how_to_optimize_gemm_amd import q8
    rng = np.random.default_rng(21)
    w = rng.uniform(-1, 1, (130, 200)).astype(np.float32)
    bias = rng.uniform(-1, 1, 130).astype(np.float32)
    qw, db = q8.QWeight(torch.from_numpy(w).cuda()), torch.from_numpy(bias).cuda()
    x = torch.zeros((77, 200), device="cuda")
    y = torch.full((77, 130), float("nan"), device="cuda")
    side = _side_stream()
    with torch.cuda.stream(side):
        q8.qlinear(x, qw, db, "relu", out=y)
    side.synchronize()
    graph = _capture(side, lambda: q8.qlinear(x, qw, db, "relu", out=y))
    for rep in range(3):
        a = (rng.standard_normal((77, 200)) * (rep + 1)).astype(np.float32)
        x.copy_(torch.from_numpy(a))
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        eager = q8.qlinear(x.clone(), qw, db, "relu").cpu().numpy()
        assert same_bits(got, eager), (rep, first_difference(got, eager))
        assert same_bits(got, R.qlinear_ref(a, w, bias, True)), rep
    del graph


def test_the_module_is_the_contract_and_lies_within_the_quantisation_bound():
    """QLinear.from_float(nn.Linear(96, 80)) on a (2, 5, 96) input equals qlinear_ref, and lies within the analytic bound of
    the fp32 layer.

    The bound.  For a vector v with finite elements, a = max|v|, s = 127 / a: v_k * s lies in [-127, 127], so rint moves it by
    at most 1/2 and never clamps: |Q(v)_k / s - v_k| <= 1 / (2 s) = a / 254 =: d(v).  Write xq_k = Q(x)_k / sx = x_k + ex_k and
    wq_k = Q(w)_k / sw = w_k + ew_k with |ex_k| <= d(x), |ew_k| <= d(w).  The exact layer on the quantised operands differs from
    the exact layer by
        |sum_k xq_k wq_k - sum_k x_k w_k| = |sum_k (x_k ew_k + ex_k w_k + ex_k ew_k)|
                                         <= d(w) sum_k |x_k| + d(x) sum_k |w_k| + K d(x) d(w)                      (tight)
    and, since max|v| <= sum_k |v_k| =: S(v) and |ex_k| <= |x_k| as well (an element that rounds to 0 is off by itself, any
    other by at most half a step, which is below it), sum_k |ex_k ew_k| <= S(x) d(w):
                                         <= S(x) S(w) (1/254 + 1/254 + 1/254) < S(x) S(w) (1/127 + 1/127 + 1/127^2)  (the issue's)
    with S(x) S(w) the product of the two rows' absolute sums.  Both are asserted.  fp32 slack: y is three roundings of that
    exact value (and two rounded reciprocals) and the fp32 layer a K-term fp32 sum: (K + 8) 2^-24 (sum_k |x_k w_k| (1 + 3/127) + |b_j|)."""
    import torch
    from how_to_optimize_gemm_amd import q8
    torch.manual_seed(4)
    linear = torch.nn.Linear(96, 80).cuda()
    layer = q8.QLinear.from_float(linear)
    x = torch.randn(2, 5, 96, device="cuda")
    y = layer(x)
    assert tuple(y.shape) == (2, 5, 80)
    xn, wn, bn = x.reshape(10, 96).cpu().numpy(), linear.weight.detach().cpu().numpy(), linear.bias.detach().cpu().numpy()
    got = y.reshape(10, 80).cpu().numpy()
    want = R.qlinear_ref(xn, wn, bn)
    assert same_bits(got, want), first_difference(got, want)
    with torch.no_grad():
        fp32 = linear(x).reshape(10, 80).cpu().numpy().astype(np.float64)
    ax, aw = np.abs(xn).astype(np.float64), np.abs(wn).astype(np.float64)
    dx, dw = ax.max(axis=1) / 254, aw.max(axis=1) / 254
    tight = ax.sum(axis=1)[:, None] * dw[None, :] + dx[:, None] * aw.sum(axis=1)[None, :] + 96 * dx[:, None] * dw[None, :]
    issue = ax.sum(axis=1)[:, None] * aw.sum(axis=1)[None, :] * (2 / 127 + 1 / 127 ** 2)
    slack = (96 + 8) * 2.0 ** -24 * ((ax @ aw.T) * (1 + 3 / 127) + np.abs(bn)[None, :])
    err = np.abs(got.astype(np.float64) - fp32)
    assert (err <= tight + slack).all(), (err - tight - slack).max()
    assert (err <= issue + slack).all(), (err - issue - slack).max()
    # ReLU in the module, no bias, and what it refuses
    plain = torch.nn.Linear(96, 80, bias=False).cuda()
    relu = q8.QLinear.from_float(plain, activation="relu")
    assert relu.bias is None
    assert same_bits(relu(x).reshape(10, 80).cpu().numpy(), R.qlinear_ref(xn, plain.weight.detach().cpu().numpy(), None, True))
    import how_to_optimize_gemm_amd as H
    with pytest.raises(H.MMultError):
        layer(x.clone().requires_grad_())
    with pytest.raises(H.MMultError):
        q8.QLinear(96, 80)(x)   # no weight prepared


def test_reserve_sizes_the_scratch_for_a_captured_call_larger_than_any_eager_one():
    """What QWeight.reserve is for: an eager 8-row call loads the kernels (8 and 64 rows are both guarded: one instantiation),
    reserve(64), then a 64-row call that never ran eagerly is captured and replayed twice on new x."""
    import torch
    from how_to_optimize_gemm_amd import q8
    rng = np.random.default_rng(29)
    w = rng.uniform(-1, 1, (40, 36)).astype(np.float32)
    qw = q8.QWeight(torch.from_numpy(w).cuda())
    xs, xl = torch.zeros((8, 36), device="cuda"), torch.zeros((64, 36), device="cuda")
    ys, yl = torch.full((8, 40), float("nan"), device="cuda"), torch.full((64, 40), float("nan"), device="cuda")
    side = _side_stream()
    with torch.cuda.stream(side):
        q8.qlinear(xs, qw, out=ys)   # the eager warm-up: sizes the scratch for 8 rows
    side.synchronize()
    with torch.cuda.stream(side):
        qw.reserve(64)
    side.synchronize()
    graph = _capture(side, lambda: q8.qlinear(xl, qw, out=yl))
    for rep in range(2):
        a = (rng.standard_normal((64, 36)) * (rep + 1)).astype(np.float32)
        xl.copy_(torch.from_numpy(a))
        yl.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got, want = yl.cpu().numpy(), R.qlinear_ref(a, w)
        assert same_bits(got, want), (rep, first_difference(got, want))
    del graph


def test_time_qlinear_leaves_the_contract_in_y_and_returns_a_time(cus):
    import torch
    from how_to_optimize_gemm_amd import q8
    rng = np.random.default_rng(31)
    x = rng.standard_normal((37, 300)).astype(np.float32)
    w = rng.uniform(-1, 1, (50, 300)).astype(np.float32)
    bias = rng.uniform(-1, 1, 50).astype(np.float32)
    qw, dx, db = q8.QWeight(torch.from_numpy(w).cuda()), torch.from_numpy(x).cuda(), torch.from_numpy(bias).cuda()
    y = torch.full((37, 50), float("nan"), device="cuda")
    ms = q8.time_qlinear(dx, qw, db, "relu", out=y, warmup=1, reps=3)
    torch.cuda.synchronize()
    got, want = y.cpu().numpy(), R.qlinear_ref(x, w, bias, True)
    assert same_bits(got, want), first_difference(got, want)
    assert math.isfinite(ms) and ms > 0, ms


def test_the_module_takes_a_strided_last_dimension_and_a_vector():
    """QLinear.forward: an input whose last dimension is not unit stride goes through contiguous(); a 1-D input of in_features
    gives a 1-D output."""
    import torch
    from how_to_optimize_gemm_amd import q8
    torch.manual_seed(6)
    linear = torch.nn.Linear(96, 80).cuda()
    layer = q8.QLinear.from_float(linear, activation="relu")
    wn, bn = linear.weight.detach().cpu().numpy(), linear.bias.detach().cpu().numpy()
    x = torch.randn(96, 10, device="cuda").t()
    assert tuple(x.shape) == (10, 96) and x.stride(1) != 1
    y = layer(x)
    assert tuple(y.shape) == (10, 80)
    want = R.qlinear_ref(x.cpu().numpy(), wn, bn, True)
    assert same_bits(y.cpu().numpy(), want), first_difference(y.cpu().numpy(), want)
    v = torch.randn(96, device="cuda")
    y = layer(v)
    assert tuple(y.shape) == (80,)
    want = R.qlinear_ref(v.cpu().numpy()[None, :], wn, bn, True)[0]
    assert same_bits(y.cpu().numpy(), want), first_difference(y.cpu().numpy(), want)
