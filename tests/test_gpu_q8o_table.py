"""The int8-output layer's four kernels (libmmult_hip_q8o.so, qlinear_s8o_kernel at 128x128 and 256x256, whole and guarded) at
the shapes where tiled kernels go wrong, byte for byte against tests/qchain_ref.py: the sibling of test_gpu_qlinear.py's case
table, on top of test_gpu_qchain.py's helpers.

A case is (rows, out, in_, ldq_pad, off_x, ldyq, off_y): x's int8 rows have the pitch `in_` rounded up to 4 plus ldq_pad and
start off_x bytes past a 16-byte boundary, their pad bytes poisoned with 0x55; yq's rows are ldyq bytes apart and start off_y
bytes past a 16-byte boundary, in a buffer poisoned with 0x55 in front of the window, behind every row and behind the last row
(16 bytes of slack in front, 64 behind).  s8o_cases has the table (tests/test_q8o_coverage.py holds the classes it promises, on
the CPU); one test id per (tile, guarded, case) runs the case's epilogues on deep_problem's inputs, whose every 128-byte slice of
k moves the expected BYTES -- requantisation can hide a small error of the sums, so the condition is stated on the bytes.

Behind the table: the operands as a caller may make them (rows that hold -128, row factors that are no quantiser's reciprocal,
sums beyond 2^24, rows with nothing behind them at bases 4, 8 and 12 bytes past 16) through both entry points that take int8
rows, mmh_q8o_linear and mmh_q8_linear_s8; and the output scale at every finite value the header allows, and at the non-finite
ones for which it promises only that nothing outside the window is written."""
import collections
import functools

import numpy as np
import pytest

import qchain_ref as Q
import qlinear_ref as R
import test_gpu_qchain as C
from bitcmp import first_difference, same_bits
from gpu_operands import _padded, cus_fixture, handle_fixture
from test_gpu_qlinear import KS_256, KS_256_EDGE, KS_Q8, THIN, thin_256

pytestmark = pytest.mark.gpu

amm = handle_fixture()        # asked for the device's CU count only
cus = cus_fixture("amm")

S8oCase = collections.namedtuple("S8oCase", "rows out in_ ldq_pad off_x ldyq off_y")
CLASSES = [(r.tile, r.edge) for r in C.Q8O_INSTANTIATIONS]
X_LAYOUTS = [(pad, off) for pad in (0, 4, 8, 12) for off in (0, 4, 8, 12)]   # (ldq_pad, off_x)
# bias and ReLU are runtime arguments of one kernel: the 128 classes run all four, the 256 classes the two that set each once
EPILOGUES = {128: C.EPILOGUES, 256: [(True, False), (False, True)]}


def x_layout(i):
    """The i-th x layout of a rotation that reaches all sixteen in sixteen steps; the first is dense."""
    return X_LAYOUTS[5 * i % 16]


def pitch(out, kind):
    """The smallest pitch of at least out + 4 bytes that is odd (kind 0), 2 modulo 4 (kind 1), 0 modulo 4 (kind 2)."""
    p = out + 4
    return p + (p + 1) % 2 if kind == 0 else p + (2 - p % 4) % 4 if kind == 1 else p + -p % 4


def symbol_of(tile, edge):
    return next(r.symbol for r in C.Q8O_INSTANTIATIONS if (r.tile, r.edge) == (tile, edge))


def s8o_cases(tile, edge, cu_count):
    """The S8oCases of a (tile, guarded) class; the same number on every device."""
    cases = []
    if tile == 128 and not edge:
        # K depth and every tail behind the unguarded dword store; pitches at and above out, bases 0 - 12 bytes past 16
        cases += [S8oCase(128, 128, k, *x_layout(i), 128 + (0, 4, 16)[i % 3], (0, 4, 8, 12)[i % 4]) for i, k in enumerate(KS_Q8)]
        cases += [S8oCase(128, 128, 512, 0, 0, 128, 0)]                       # fully dense
        # grids: 9 tiles (no multiple of the 8 XCDs), 1 x 17, 17 x 1
        cases += [S8oCase(384, 384, 64, *x_layout(1), 384 + 16, 4), S8oCase(128, 2176, 64, *x_layout(2), 2176, 8),
                  S8oCase(2176, 128, 64, *x_layout(3), 128 + 4, 12)]
    elif tile == 128:
        cases += [S8oCase(c.rows, c.out, c.in_, 4, 0, c.ldyq, c.off) for c in C.store_cases()]
        cases += [S8oCase(128 + THIN[i % 7], 128 + THIN[(i + 3) % 7], k, *x_layout(i), pitch(128 + THIN[(i + 3) % 7], i % 3), i % 4)
                  for i, k in enumerate(KS_Q8)]
        cases += [S8oCase(637, 379, 65, *x_layout(1), 379 + 4, 1),            # 5 x 3 tiles, an odd pitch
                  S8oCase(100, 2177, 64, *x_layout(2), 2180, 2), S8oCase(2177, 100, 64, *x_layout(3), 102, 0),   # 1 x 18, 18 x 1
                  S8oCase(1, 1, 1, 4, 4, 5, 3), S8oCase(1, 130, 257, 8, 12, 136, 0)]   # one row at a pitch of its own
    elif not edge:
        m, n, _ = C.shapes_256(cu_count)[0]
        cases += [S8oCase(m, n, k, *x_layout(i), n + (0, 4, 16)[i % 3], (0, 4, 8, 12)[i]) for i, k in enumerate(KS_256)]
    else:
        m, n, _ = C.shapes_256(cu_count)[0]
        # pitches 0 modulo 4, odd, 2 modulo 4, ...; bases 1, 2, 3, 0, ...: case 3 is ragged (17 columns) in dwords
        for i, k in enumerate(KS_256_EDGE):
            rows, out = thin_256(THIN[i], THIN[(i + 3) % 7], cu_count)
            cases.append(S8oCase(rows, out, k, *x_layout(i), pitch(out, (i + 2) % 3), (i + 1) % 4))
        cases += [S8oCase(m, n, 513, 4, 4, n + 4, 1),                         # whole tiles guarded by the base alone
                  S8oCase(m, n, 513, 8, 0, n + 1, 0)]                         # ... by the pitch alone
    return cases


def ldq_of(c):
    return ((c.in_ + 3) & ~3) + c.ldq_pad


# ---- inputs on which an error shows in the bytes ------------------------------------------------------------------------
def every_slice_moves_the_bytes(p):
    """Zeroing any one 128-byte slice of k changes at least 90 % of the expected bytes of the (bias, no ReLU) epilogue (of the
    first 128 x 128 of them)."""
    w, bias, xq, rx, acc, rw, so = p
    qw, _, _ = R.quantize_rows_ref(w[:128])
    xq, rx, rw, bias, so, acc = xq[:128], rx[:128], rw[:128], bias[:128], so[:128], acc[:128, :128]
    want = Q.requant_ref(R.epilogue_ref(acc, rx, rw, bias, False), so)
    for k0 in range(0, xq.shape[1], 128):
        less = acc - R.int_sums(xq[:, k0:k0 + 128], qw[:, k0:k0 + 128])
        changed = float((Q.requant_ref(R.epilogue_ref(less, rx, rw, bias, False), so) != want).mean())
        assert changed >= 0.9, (xq.shape, qw.shape, k0, changed)


@functools.lru_cache(maxsize=1)
def deep_problem(rows, out, in_):
    """test_gpu_qchain.problem()'s distributions, scale rule and per-row output scale; the last column of every row of x and of
    w is plus or minus that row's maximum.  Asserts on the host that the expected bytes are no constant and do not saturate
    (shapes of a thousand outputs, as problem()'s callers do) and that every slice of k moves them.  Returns (problem()'s tuple,
    the expected bytes of the (bias, no ReLU) epilogue)."""
    rng = np.random.default_rng(rows * 7 + out * 3 + in_ + 3)
    x = (rng.standard_normal((rows, in_)) * 3).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, (out, in_)).astype(np.float32)
    bias = rng.uniform(-4, 4, out).astype(np.float32)
    for v in (x, w):
        v[:, -1] = np.abs(v).max(axis=1) * rng.choice(np.array([-1, 1], np.float32), v.shape[0])
    xq, _, rx = R.quantize_rows_ref(x)
    qw, _, rw = R.quantize_rows_ref(w)
    acc = R.int_sums(xq, qw)
    y = R.epilogue_ref(acc, rx, rw, bias, False)
    p = (w, bias, xq, rx, acc, rw, C.scales_of(y))
    want = Q.requant_ref(y, p[6])
    if rows * out >= 1000:
        count = np.bincount(want.view(np.uint8).reshape(-1), minlength=256)   # (of byte patterns: 129 and 127 are -127 and 127)
        values, clamped = int(np.count_nonzero(count)), float(count[127] + count[129]) / want.size
        assert values >= 100 and clamped < 0.01, ((rows, out, in_), values, clamped)
    every_slice_moves_the_bytes(p)
    return p, want


@pytest.mark.parametrize("tile,edge,index", [(t, e, i) for t, e in CLASSES for i in range(len(s8o_cases(t, e, 256)))],
                         ids=lambda v: {False: "whole", True: "guarded"}[v] if isinstance(v, bool) else str(v))
def test_every_case_of_the_q8o_table_is_the_contract_in_its_epilogues(tile, edge, index, cus):
    """K depth and tails, thin last tiles, grids, pitches and bases of both operands (s8o_cases) on deep_problem's inputs: the
    bytes are the reference's, the launch is the plan's text and the class's symbol, nothing outside rows x out bytes changed."""
    import torch
    from how_to_optimize_gemm_amd import q8
    cases = s8o_cases(tile, edge, cus)
    assert len(cases) == len(s8o_cases(tile, edge, 256))
    c = cases[index]
    p, want = deep_problem(c.rows, c.out, c.in_)
    qw = q8.QWeight(torch.from_numpy(p[0]).cuda())
    for e in EPILOGUES[tile]:
        C.check_s8o((c.rows, c.out, c.in_), p, qw, *e, c.ldyq, c.off_y, symbol_of(tile, edge), cus, want if e == (True, False) else None,
                    x_pad=c.ldq_pad, x_off=c.off_x)
    qw.close()


# ---- the operands as a caller may make them -----------------------------------------------------------------------------
_B = {False: "false", True: "true"}
S8O_EDGE, S8O_WHOLE = "qlinear_s8o_kernel<128,128,4,true>", "qlinear_s8o_kernel<128,128,4,false>"


def check_rows(xq, rx, w, bias, so, cu_count, x_pad=4, x_off=0, whole=False, entries=("s8o", "s8")):
    """Caller-made int8 rows through both entry points that take them, with and without ReLU: mmh_q8o_linear into poisoned
    bytes (guarded: an odd pitch, a base 1 byte off) against qlinear_s8_ref(..., so), and mmh_q8_linear_s8 into NaN-padded
    floats (guarded: an odd leading dimension, a base 4 bytes past 16) against qlinear_s8_ref(..., so=None).  bias None: no sum."""
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, out = xq.shape[0], w.shape[0]
    qw = q8.QWeight(torch.from_numpy(w).cuda())
    db = None if bias is None else torch.from_numpy(bias).cuda()
    ldyq, off_y = (out, 0) if whole else (out + 7 + out % 2, 1)
    ldy, off_f = (out + 4, 4) if whole else (out + 1, 1)
    for relu in (False, True):
        if "s8o" in entries:
            want = Q.qlinear_s8_ref(xq, rx, w, bias, relu, so)
            got, untouched, launched = C.run_s8o(qw, xq, rx, bias, relu, so, ldyq, off_y, x_pad, x_off)
            assert launched == Q.plan_text_s8o(rows, out, ldyq, off_y, cu_count) and (S8O_WHOLE if whole else S8O_EDGE) in launched, launched
            assert np.array_equal(got, want), (relu, launched, int((got != want).sum()), np.argwhere(got != want)[:4])
            assert untouched, (launched, "wrote outside yq's rows x out bytes")
        if "s8" in entries:
            want = Q.qlinear_s8_ref(xq, rx, w, bias, relu)
            yflat, yv = _padded(rows, out, ldy, off_f)
            q8.qlinear(C.device_rows(xq, rx, x_pad, x_off), qw, db, "relu" if relu else None, out=yv[:, :out])
            launched = q8.last_launch()
            torch.cuda.synchronize()
            got = yv[:, :out].cpu().numpy()
            assert f"qlinear_s8_kernel<128,128,4,{_B[not whole]},{_B[bias is not None]},{_B[relu]}>" in launched, launched
            assert same_bits(got, want), (relu, launched, first_difference(got, want))
            assert bool(torch.isnan(yv[:, out:]).all()) and bool(torch.isnan(yflat[:off_f]).all()) and \
                bool(torch.isnan(yflat[off_f + rows * ldy:]).all()), (launched, "wrote outside y's window")
    qw.close()


def int8_rows(rng, shape):
    """Random int8 over the full range with -128 planted at about 1 / 64 of the positions (tests/int8_ops.py's _int8)."""
    x = rng.integers(-128, 128, shape, dtype=np.int8)
    x.reshape(-1)[rng.integers(0, x.size, max(1, x.size // 64))] = -128
    return x


def minus128_problem(rows, out, in_):
    """Rows no quantiser makes: the full int8 range with -128 planted, row 1 all -128, against a weight whose channel 2 has the
    image all +-127; arbitrary positive row factors; the output scales of problem()'s rule."""
    rng = np.random.default_rng(rows + out + in_ + 128)
    xq = int8_rows(rng, (rows, in_))
    xq[1] = -128
    w = rng.uniform(-0.5, 0.5, (out, in_)).astype(np.float32)
    w[2] = np.float32(0.3) * rng.choice(np.array([-1, 1], np.float32), in_)
    bias = rng.uniform(-4, 4, out).astype(np.float32)
    rx = rng.uniform(0.01, 0.05, rows).astype(np.float32)
    qw, _, rw = R.quantize_rows_ref(w)
    acc = R.int_sums(xq, qw)
    assert (np.abs(qw[2]) == 127).all() and (xq == -128).mean() > 1 / 128 and abs(int(acc[1, 2])) % 128 == 0 and acc[1, 2] != 0
    so = C.out_scales(acc, rx, rw, bias)
    want = Q.requant_ref(R.epilogue_ref(acc, rx, rw, bias, False), so)
    assert len(np.unique(want)) >= 100 and (np.abs(want) == 127).mean() < 0.01, len(np.unique(want))
    return xq, rx, w, bias, so


@pytest.mark.parametrize("shape,whole", [((37, 70, 257), False), ((128, 128, 513), True)], ids=["guarded", "whole"])
def test_rows_that_hold_minus_128(shape, whole, cus):
    """-128 is a legal byte of a caller's rows (the quantisers never write it): both entry points give the reference's sums."""
    check_rows(*minus128_problem(*shape), cus, whole=whole)


F32_DENORMAL = np.float32(1e-40)
RX_SPECIAL = np.array([0.0, -0.0, F32_DENORMAL, R.F32_MAX, -0.03, np.inf, np.nan], np.float32)


def rx_problem():
    """(16, 29, 40): the row factors of RX_SPECIAL with so = 1 (rows 0 - 6) and with so = 0.37 (rows 7 - 13), two plain rows;
    weight channels 3 and 11 are zero, so their sums are exactly 0 -- times an infinite row factor: NaN, the byte 0."""
    rng = np.random.default_rng(40)
    rows, out, in_ = 16, 29, 40
    xq = rng.integers(-127, 128, (rows, in_), dtype=np.int8)
    w = rng.uniform(-1, 1, (out, in_)).astype(np.float32)
    w[[3, 11]] = 0.0
    bias = rng.uniform(-4, 4, out).astype(np.float32)
    rx = np.concatenate([RX_SPECIAL, RX_SPECIAL, np.array([0.02, 0.05], np.float32)])
    so = np.concatenate([np.full(7, 1.0, np.float32), np.full(7, 0.37, np.float32), np.array([1.0, 0.37], np.float32)])
    qw, _, rw = R.quantize_rows_ref(w)
    acc = R.int_sums(xq, qw)
    live = np.delete(np.arange(out), [3, 11])
    assert (acc[:, live] != 0).all() and not acc[:, [3, 11]].any()
    want = Q.requant_ref(R.epilogue_ref(acc, rx, rw, bias, False), so)
    # what the contract says of them: a NaN row factor gives 0 everywhere, an infinite one +-127 by the sum's sign and 0 where
    # the sum is 0, FLT_MAX the same but the bias alone (rounded) where the sum is 0
    assert not want[[6, 13]].any()
    assert (want[5][live] == 127 * np.sign(acc[5][live])).all() and not want[5][[3, 11]].any()
    assert (want[3][live] == 127 * np.sign(acc[3][live])).all() and (want[3][[3, 11]] == np.rint(bias[[3, 11]])).all()
    assert (want[0] == want[1]).all() and (want[0] == Q.requant_ref(bias[None, :], so[:1])[0]).all()
    return xq, rx, w, bias, so


def test_row_factors_that_are_no_reciprocal_of_a_quantisers_scale(cus):
    """rx is the caller's: in a chain it is fl(1 / so) of the layer before, any float.  0, -0, a denormal, FLT_MAX, a negative
    value, +inf and NaN at non-zero sums and at sums that are exactly 0."""
    xq, rx, w, bias, so = rx_problem()
    check_rows(xq, rx, w, bias, so, cus)
    # without a bias the fp32 output keeps what a denormal row factor leaves of the sums (with one, the bias absorbs it)
    want = Q.qlinear_s8_ref(xq, rx, w)
    assert np.count_nonzero(want[2]) == want.shape[1] - 2 and (np.abs(want[2]) < 1e-33).all()
    check_rows(xq, rx, w, None, so, cus, entries=("s8",))


def large_sums_problem():
    """test_gpu_qlinear's test_large_sums_round_to_nearest_even, its last step: (64, 64, 2048), every |element| its row's
    maximum but one per row of x at 2 / 127 of it, every other channel of w negated: odd sums beyond +-2^24, which (float)acc
    has to round.  The output scales of problem()'s rule."""
    rng = np.random.default_rng(11)
    x = np.where(rng.random((64, 2048)) < 0.05, -1.5, 1.5).astype(np.float32) * rng.uniform(0.5, 2, (64, 1)).astype(np.float32)
    w = np.where(rng.random((64, 2048)) < 0.05, -0.25, 0.25).astype(np.float32) * rng.uniform(0.5, 2, (64, 1)).astype(np.float32)
    x[0], w[0] = 1.5, 0.25
    x[:, 5] *= np.float32(2.0 / 127.0)
    w[::2] = -w[::2]
    xq, _, rx = R.quantize_rows_ref(x)
    qw, _, rw = R.quantize_rows_ref(w)
    acc = R.int_sums(xq, qw)
    inexact = acc.astype(np.float32).astype(np.int64) != acc
    assert inexact.sum() > 1000 and inexact[acc > 1 << 24].sum() > 100 and inexact[acc < -(1 << 24)].sum() > 100
    bias = rng.uniform(-4, 4, 64).astype(np.float32)
    so = C.out_scales(acc, rx, rw, bias)
    want = Q.requant_ref(R.epilogue_ref(acc, rx, rw, bias, False), so)
    assert (np.abs(want) == 127).mean() < 0.01 and len(np.unique(want)) >= 100, len(np.unique(want))
    return xq, rx, w, bias, so


def test_sums_beyond_2_to_the_24_through_the_int8_output(cus):
    check_rows(*large_sums_problem(), cus)


@pytest.mark.parametrize("in_", [516, 513])
def test_rows_with_nothing_behind_them_at_bases_past_16(in_, cus):
    """ldq == in_ at in_ = 516: the row's last dword is the last of its pitch; in_ = 513 at ldq = 516: three poisoned bytes and
    nothing else.  Three trips of the K loop, x 4, 8 and 12 bytes past a 16-byte boundary."""
    p = C.problem(37, 70, in_)
    w, bias, xq, rx, acc, rw, so = p
    for off in (4, 8, 12):
        check_rows(xq, rx, w, bias, so, cus, x_pad=0, x_off=off)


# ---- the output scale ---------------------------------------------------------------------------------------------------
FINITE_SCALES = np.array([0.0, -0.0, -1.0, -0.5, 2.0 ** -140, R.F32_MAX, 1e30, 1e-30], np.float32)


def scale_problem():
    """(18, 29, 40) with the bias C.BIASES.  Integer weights whose every channel holds 127 (the image is the weight, rw = 1).
    Even rows: x = 0 and rx = -1, so y is the bias itself -- its ties, +-inf, NaN, and -0 (the sum is -0); odd rows: small
    integers with rx = 1 / 64, so y = acc / 64 + bias exactly.  Rows 2 i and 2 i + 1 take FINITE_SCALES[i]; the last two 1."""
    rng = np.random.default_rng(29)
    rows, out, in_ = 18, len(C.BIASES), 40
    w = rng.integers(-127, 128, (out, in_)).astype(np.float32)
    w[:, 7] = 127.0
    xq = rng.integers(-3, 4, (rows, in_), dtype=np.int8)
    xq[::2] = 0
    rx = np.where(np.arange(rows) % 2 == 0, -1.0, 1 / 64).astype(np.float32)
    so = np.concatenate([np.repeat(FINITE_SCALES, 2), np.ones(2, np.float32)])
    qw, _, rw = R.quantize_rows_ref(w)
    assert np.array_equal(qw, w) and (rw == 1).all()
    acc = R.int_sums(xq, qw)
    y = R.epilogue_ref(acc, rx, rw, C.BIASES, False)
    assert same_bits(y[::2], np.tile(C.BIASES, (rows // 2, 1))) and np.signbit(y[0, 16]) and (acc[1::2] != 0).mean() > 0.9
    assert np.array_equal(y[1::2][:, :11].astype(np.float64), acc[1::2][:, :11] / 64 + C.BIASES[:11].astype(np.float64))
    # rows 4 - 7 (so = -1, -0.5) and 16, 17 (so = 1): ties of both parities inside the range, values that clamp on both sides
    with np.errstate(invalid="ignore"):
        t = (y.astype(np.float64) * so.astype(np.float64)[:, None])[[4, 5, 6, 7, 16, 17]]
    t = t[np.isfinite(t)]
    ties = t[(np.abs(t) < 127) & (t - np.floor(t) == 0.5)]
    assert (np.floor(ties) % 2 == 0).any() and (np.floor(ties) % 2 == 1).any() and (t > 127.5).any() and (t < -127.5).any()
    return xq, rx, w, C.BIASES, so


def test_every_finite_output_scale_is_the_contract(cus):
    """0, -0, negative, denormal, FLT_MAX, one that overflows y * so and one that underflows it: the bytes are requant_ref's,
    which restates quantize_one including what fmaxf / fminf do with inf * 0 (tests/test_qchain_ref.py spells those out)."""
    check_rows(*scale_problem(), cus, entries=("s8o",))


def test_a_non_finite_output_scale_stays_inside_the_window_and_leaves_the_other_rows_exact(cus):
    """The header's promise for +inf, -inf and NaN scales: the bytes of those rows are unspecified, nothing outside rows x out
    bytes is written, and every row with a finite scale is still exact.  The front end refuses a non-finite Python float and
    passes a tensor through."""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    xq, rx, w, bias, so = scale_problem()
    so = so.copy()
    bad = [1, 4, 7, 16]
    so[bad] = [np.inf, -np.inf, np.nan, np.inf]
    finite = np.isfinite(so)
    rows, out = xq.shape[0], w.shape[0]
    qw = q8.QWeight(torch.from_numpy(w).cuda())
    for relu in (False, True):
        for ldyq, off_y in ((out + 3, 1), ((out + 6) & ~3, 0)):   # bytes; dwords on a ragged tile
            want = Q.qlinear_s8_ref(xq, rx, w, bias, relu, np.where(finite, so, np.float32(1.0)))
            got, untouched, launched = C.run_s8o(qw, xq, rx, bias, relu, so, ldyq, off_y)
            assert S8O_EDGE in launched and untouched, (launched, "wrote outside yq's rows x out bytes")
            assert np.array_equal(got[finite], want[finite]), (relu, ldyq, np.argwhere(got[finite] != want[finite])[:4])
    rows_q = C.device_rows(xq, rx)
    for s in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(H.MMultError) as e:
            q8.qlinear(rows_q, qw, out_scale=s)
        assert e.value.status == H.ERR_INVALID_ARG
    passed = q8.qlinear(rows_q, qw, out_scale=torch.from_numpy(so).cuda())
    torch.cuda.synchronize()
    assert tuple(passed.q.shape) == (rows, out) and same_bits(passed.inv_scale.cpu().numpy(), Q.inv_scale_ref(so))
    qw.close()
