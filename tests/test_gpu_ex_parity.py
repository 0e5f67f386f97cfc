"""Every fused-epilogue instantiation of libmmult_hip.so (mmh_sgemm_ex: sgemm_mfma_dma5_ex_kernel and
sgemm_dma5_ex_streamk_kernel, csrc/sgemm_dma5.hpp EP, csrc/launch_ex.hip, csrc/launch_ex_t.hip) against the numpy expectation
of the contract, bit for bit, and the special values of the epilogue on every tile and on the naive kernel.

EX_INSTANTIATIONS has one row per instantiation: three tiles x whole / guarded x plain / chained stream-K x four operand
pairs = 48.  A row says how a caller reaches it (forced kernel, MMH_OPT_STREAMK, MMH_OPT_PERSIST, operand pair), which words
of mmh_last_launch prove that it ran, and the shapes it runs -- the ones the NN and op rows of the same tile and edge run in
tests/test_gpu_lds_dma_parity.py.  tests/test_ex_coverage.py holds the table to the symbols of the built library on the CPU.

The expectation is tests/test_gpu_ex.py's `expected` on the oracle's fused chain: numpy alone.  sgemm_naive_ex_kernel calls
the tiles' dma5_epilogue_apply, so for the epilogue it is no independent reference; numpy is the only one."""
import dataclasses
import functools
import re
from typing import Callable, Optional

import numpy as np
import pytest

from test_gpu_ex import COL, NONE, RELU, ROW, dev, expected
from test_gpu_lds_dma_parity import (K2W_SK, K2W_TILES, OP_LAYOUTS, _case, _ld, _padded, _plain_shapes, _special_shapes,
                                     _streamk_shapes, first_difference, same_bits)

pytestmark = pytest.mark.gpu

# ---- the table --------------------------------------------------------------------------------------------------------
EX_OPS = {0: (0, 0), **OP_LAYOUTS}   # the OP template argument = transa | transb << 1 -> (transa, transb)
EX_FAMILY_RE = re.compile(r"^(?P<family>sgemm_mfma_dma5_ex_kernel|sgemm_dma5_ex_streamk_kernel)<(?P<bm>\d+),(?P<bn>\d+),32,\d+,\d+,3,"
                          r"(?P<edge>true|false),\d+,2,(?P<op>[0-3])>$")


def pair_name(ops):
    return "NT"[ops[0]] + "NT"[ops[1]]


def ex_tag(ops, alpha, beta, mode, act):
    """What the description of an `ex` launch ends in (ex_tag, csrc/launch_dma5.hpp)."""
    words = [w for on, w in ((np.float32(alpha) != 1, "alpha"), (np.float32(beta) != 0, "beta"), (mode == COL, "bias(col)"),
                             (mode == ROW, "bias(row)"), (act == RELU, "relu")) if on]
    return f", operands {pair_name(ops)}, epilogue " + (" ".join(words) or "identity")


def _ex_symbols():
    for t in K2W_SK:
        for e in ("false", "true"):
            for op in EX_OPS:
                yield f"sgemm_mfma_dma5_ex_kernel<{t},{e},{K2W_TILES[t]},{op}>"
                yield f"sgemm_dma5_ex_streamk_kernel<{t},{e},{K2W_TILES[t]},{op}>"


@dataclasses.dataclass(frozen=True)
class ExInst:
    symbol: str
    kernel: str          # forced kernel (MMult.set_kernel)
    streamk: int         # MMH_OPT_STREAMK: 0 = plain launches only, 2 = stream-K whenever the count is ragged
    persist: int         # MMH_OPT_PERSIST: whole rounds of the persistent grid run persistent too
    ops: tuple           # (transa, transb)
    head: str            # what mmh_last_launch starts with ...
    markers: tuple       # ... the words it must hold ...
    absent: tuple        # ... and must not (it ends in ex_tag of the epilogue that ran)
    shapes: Callable     # cus -> [(m, n, k, whole_rounds)]

    @property
    def bm_bn(self):
        m = EX_FAMILY_RE.match(self.symbol)
        return int(m["bm"]), int(m["bn"])

    @property
    def guarded(self):
        return "guarded" in self.markers


def _ex_row(symbol):
    m = EX_FAMILY_RE.match(symbol)
    assert m, symbol
    fam, bm, bn, edge = m["family"], int(m["bm"]), int(m["bn"]), m["edge"] == "true"
    sk = "streamk" in fam
    on, off = ["persistent", "chained parts"], []
    if not sk:
        on, off = off, on
    (on if edge else off).append("guarded")
    shapes = _streamk_shapes(bm, bn, edge, True) if sk else _plain_shapes(bm, bn, edge)
    return ExInst(symbol=symbol, kernel=f"mfma_{bm}x{bn}_dma5", streamk=2 if sk else 0, persist=1 if sk else 0, ops=EX_OPS[int(m["op"])],
                  head=f"{fam}<{bm},{bn}>", markers=tuple(on), absent=tuple(off), shapes=shapes)


def _ex_order(inst):   # the four operand rows of a tile, edge and launch form next to each other: they share shapes and oracle results
    return inst.bm_bn + (inst.guarded, inst.streamk, inst.symbol)


EX_INSTANTIATIONS = sorted((_ex_row(s) for s in _ex_symbols()), key=_ex_order)

# name: alpha, beta, bias mode, activation -- every switch of dma5_epilogue_apply on in the first, off in the last.  beta == 0
# runs over a C window of NaN: it must not be read.
ROW_EPILOGUES = {"all": (-1.3, 0.5, COL, RELU), "row_bias": (1.0, 0.0, ROW, 0), "identity": (1.0, 0.0, NONE, 0)}


# ---- running a row ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _ex_case(m, n, k):
    """_case's inputs and chain s of a shape, a bias per column and per row, and the expectation of every row epilogue; C and
    the expectations on the device too, where the rows compare (the four operand rows that run the shape reuse all of it)."""
    a, b, c0, s, _ = _case(m, n, k)
    rng = np.random.default_rng(3 * m + 5 * n + k)
    bias = {NONE: None, COL: rng.uniform(-1, 1, n).astype(np.float32), ROW: rng.uniform(-1, 1, m).astype(np.float32)}
    want = {name: expected(s, alpha, beta, c0, bias[mode], mode, act) for name, (alpha, beta, mode, act) in ROW_EPILOGUES.items()}
    assert same_bits(want["identity"], s)   # (1 * s = s: the identity's expectation IS the oracle's chain)
    return a, b, dev(c0), bias, want, {name: dev(w) for name, w in want.items()}


def same_bits_on_device(got, want):
    """same_bits on device tensors."""
    import torch
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and \
        torch.equal(got.view(torch.int32).masked_fill(nan, 0), want.view(torch.int32).masked_fill(nan, 0))


def run_ex(mm, ops, a, b, alpha, beta, c_init, bias, mode, act, guarded):
    """C = act(alpha op(A) op(B) + beta C + bias) through mmh_sgemm_ex on NaN-padded operands laid out as
    test_gpu_lds_dma_parity.run_gemm lays them: guarded -- odd leading dimensions, bases and the bias 4 bytes past 16-byte
    alignment; otherwise leading dimensions that are multiples of 4 and 16-byte aligned bases.  c_init: a device tensor, or
    None: C's window is NaN too.  Returns (C's window on the device, whether anything outside it was written, the launch string)."""
    import torch
    import how_to_optimize_gemm_amd as H
    m, k = a.shape
    n = b.shape[1]
    off = 1 if guarded else 4
    ta, tb = ops
    sa = np.ascontiguousarray(a.T) if ta else a
    sb = np.ascontiguousarray(b.T) if tb else b
    lda, ldb, ldc = _ld(sa.shape[1], guarded), _ld(sb.shape[1], guarded), _ld(n, guarded)
    _, av = _padded(*sa.shape, lda, off, sa)
    _, bv = _padded(*sb.shape, ldb, off, sb)
    cflat, cv = _padded(m, n, ldc, off)
    if c_init is not None:
        cv[:, :n] = c_init
    bias_ptr = 0
    if mode != NONE:
        _, biasv = _padded(1, len(bias), len(bias), off, bias[None, :])
        bias_ptr = biasv.data_ptr()
    mm.sgemm_ex(ta, tb, m, n, k, alpha, av.data_ptr(), lda, bv.data_ptr(), ldb, beta, cv.data_ptr(), ldc, bias_ptr, mode, act,
                torch.cuda.current_stream().cuda_stream)
    launched = H.last_launch()
    torch.cuda.synchronize()
    untouched = bool(torch.isnan(cv[:, n:]).all()) and bool(torch.isnan(cflat[:off]).all()) and \
        bool(torch.isnan(cflat[off + m * ldc:]).all())
    return cv[:, :n], untouched, launched


def check_launch(launched, head, markers, absent, tag, where):
    assert launched.startswith(head), (where, head, launched)
    for word in markers:
        assert word in launched, (where, word, launched)
    for word in absent:
        assert word not in launched, (where, word, launched)
    assert launched.endswith(tag), (where, tag, launched)


class _ExOptions:
    """A reach (forced kernel, MMH_OPT_STREAMK, MMH_OPT_PERSIST) on the session handle, and the defaults back afterwards."""

    def __init__(self, mm, kernel, streamk, persist):
        self.mm, self.reach = mm, (kernel, streamk, persist)

    def __enter__(self):
        import how_to_optimize_gemm_amd as H
        kernel, streamk, persist = self.reach
        self.mm.set_kernel(kernel)
        self.mm.set_streamk(streamk)
        self.mm.set_option(H.OPT_PERSIST, persist)

    def __exit__(self, *exc):
        import how_to_optimize_gemm_amd as H
        self.mm.set_option(H.OPT_PERSIST, 0)
        self.mm.set_streamk(1)
        self.mm.set_kernel("mfma")


@pytest.fixture(scope="module")
def cus(mm):
    return mm.device_info()["cu_count"]


@pytest.mark.parametrize("inst", EX_INSTANTIATIONS, ids=lambda i: i.symbol)
def test_every_ex_instantiation_returns_the_contract_bits(mm, cus, inst):
    bm, bn = inst.bm_bn
    with _ExOptions(mm, inst.kernel, inst.streamk, inst.persist):
        for m, n, k, whole_rounds in inst.shapes(cus):
            tiles = -(-m // bm) * -(-n // bn)
            a, b, c0, bias, want, want_dev = _ex_case(m, n, k)
            for name, (alpha, beta, mode, act) in ROW_EPILOGUES.items():
                where = (inst.symbol, (m, n, k), name)
                got, untouched, launched = run_ex(mm, inst.ops, a, b, alpha, beta, c0 if beta != 0 else None, bias[mode], mode, act,
                                                  inst.guarded)
                print(where, launched)
                check_launch(launched, inst.head, inst.markers, inst.absent, ex_tag(inst.ops, alpha, beta, mode, act), where)
                if inst.streamk:
                    t, g = (int(x) for x in re.search(r"(\d+) tiles on (\d+) persistent", launched).groups())
                    assert t == tiles, (where, launched)
                    assert (t % g == 0 and t >= 2 * g) if whole_rounds else t % g != 0, (where, launched)
                assert untouched, (where, "wrote outside C's window", launched)
                if not same_bits_on_device(got, want_dev[name]):   # (restated on the host for the message)
                    got = got.cpu().numpy()
                    assert same_bits(got, want[name]), (where, first_difference(got, want[name]), launched)
    assert mm.streamk_timeouts() == 0


# ---- special values of the epilogue -----------------------------------------------------------------------------------
TINY = np.finfo(np.float32).tiny


def _is_subnormal(x):
    return (x != 0) & (np.abs(x) < TINY)


def _neg_zero(x):
    return (x == 0) & np.signbit(x)


def _pos_zero(x):
    return (x == 0) & ~np.signbit(x)


@dataclasses.dataclass
class Block:
    name: str
    a: np.ndarray
    b: np.ndarray
    alpha: float
    beta: float
    c: Optional[np.ndarray]      # None: C's window is NaN (beta == 0 must not read it)
    bias: Optional[np.ndarray]
    mode: int
    act: int
    want: np.ndarray = None
    reaches: Callable = None     # reaches(want) asserts on the expectation alone that the block's class of values is really there

    def check_expectation(self):
        self.reaches(self.want)


@functools.lru_cache(maxsize=4)
def special_blocks(oracle, m, n, k):
    """The special-value blocks of one shape (m > 70, n > 100, k > 20), each with its expectation and a check of it.  The GPU
    test below runs them; tests/test_ex_coverage.py checks every expectation on a machine without a GPU."""
    f32 = np.float32
    a, b = oracle.harness_inputs(m, n, k, seed=1234 + m + n + k)
    rng = np.random.default_rng(m * n + k)
    c0 = rng.uniform(-1, 1, (m, n)).astype(f32)
    bias_n, bias_m = rng.uniform(-1, 1, n).astype(f32), rng.uniform(-1, 1, m).astype(f32)

    def chain(x, y):
        with np.errstate(over="ignore", invalid="ignore"):
            return oracle.ref_mmult(x, y, fma=True)

    def block(name, x, y, s, alpha, beta=0.0, c=None, bias=None, mode=NONE, act=0):
        blk = Block(name, x, y, alpha, beta, c, bias, mode, act)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            blk.want = expected(s, alpha, beta, c, bias, mode, act)
        return blk

    s = chain(a, b)
    assert np.isfinite(s).all()
    blocks = []

    # alpha == 0 is not special: 0 * s -- NaN where s is not finite, a zero of s's sign elsewhere
    a_p, b_p = a.copy(), b.copy()
    a_p[3, 5], a_p[70, 10], b_p[5, 7], b_p[20, 100] = np.inf, -np.inf, 0.0, np.nan
    s_p = chain(a_p, b_p)
    blk = block("alpha == 0", a_p, b_p, s_p, 0.0)

    def reaches(w):
        wild = ~np.isfinite(s_p)
        assert np.isnan(s_p[3, 7]) and np.isnan(s_p[:, 100]).all() and np.isinf(s_p[3]).any() and np.isinf(s_p[70]).any()
        assert np.isnan(w[wild]).all() and np.isnan(w).sum() == wild.sum() >= m + n - 1
        assert (w[~wild] == 0).all() and np.array_equal(np.signbit(w[~wild]), np.signbit(s_p[~wild]))
        assert _neg_zero(w).sum() > n and _pos_zero(w).sum() > n
    blk.reaches = reaches
    blocks.append(blk)

    # signed zero through skipped operations: rows of A all +0 give s = +0 and, with alpha = -1, r1 = -0
    zero_rows = np.arange(1, m, 4)
    a_z = a.copy()
    a_z[zero_rows] = 0.0
    s_z = chain(a_z, b)
    assert _pos_zero(s_z[zero_rows]).all()
    zero_cols = np.arange(n) % 3 == 0
    bias_neg = bias_m.copy()
    bias_neg[zero_rows] = -0.0
    bias_pos = bias_n.copy()
    bias_pos[zero_cols] = 0.0
    blk = block("signed zero, nothing switched on", a_z, b, s_z, -1.0)
    blk.reaches = lambda w: _assert(_neg_zero(w[zero_rows]).all())
    blocks.append(blk)
    blk = block("signed zero, bias -0", a_z, b, s_z, -1.0, bias=bias_neg, mode=ROW)
    blk.reaches = lambda w: _assert(_neg_zero(w[zero_rows]).all())
    blocks.append(blk)
    blk = block("signed zero, bias +0", a_z, b, s_z, -1.0, bias=bias_pos, mode=COL)
    blk.reaches = lambda w: _assert(_pos_zero(w[zero_rows][:, zero_cols]).all() and zero_cols.sum() * len(zero_rows) > 0
                                             and (w[zero_rows][:, ~zero_cols] != 0).all())
    blocks.append(blk)
    blk = block("signed zero, relu", a_z, b, s_z, -1.0, act=RELU)
    blk.reaches = lambda w: _assert(_pos_zero(w[zero_rows]).all())
    blocks.append(blk)

    # beta = -0.0 is zero: C (all NaN) is not read
    blk = block("beta == -0", a, b, s, 0.7, beta=-0.0)
    blk.reaches = lambda w: _assert(not np.isnan(w).any() and (w != 0).any())
    blocks.append(blk)

    # ReLU's classes, from C and the bias: alpha = -1 on the +0 rows gives r1 = -0, beta = 1 adds C's planted value, the bias -0
    # keeps it -- r3 is NaN, -inf, +inf, a negative subnormal, a positive subnormal, -0 by column
    planted = np.array([np.nan, -np.inf, np.inf, -2.0 ** -140, 3 * 2.0 ** -149, -0.0], dtype=f32)
    c_r = c0.copy()
    c_r[zero_rows] = planted[np.arange(n) % 6][None, :]
    blk = block("relu classes from C", a_z, b, s_z, -1.0, beta=1.0, c=c_r, bias=np.full(n, -0.0, f32), mode=COL, act=RELU)
    with np.errstate(invalid="ignore"):
        pre = expected(s_z, -1.0, 1.0, c_r, np.full(n, -0.0, f32), COL, 0)
    blk.reaches = lambda w: _relu_classes(pre, w)
    blocks.append(blk)

    # ... and from the product, ReLU alone switched on: r3 = -s with s = +0 (rows of +0), subnormals of both signs (a row whose
    # one nonzero element is 2^-100 against a row of B scaled by 2^-35), +inf, -inf and NaN (inf in A against a zero in B)
    a_q, b_q = a_z.copy(), b.copy()
    i_sub, i_inf, p_sub, p_inf = 2, 6, 4, 9
    a_q[i_sub] = 0.0
    a_q[i_sub, p_sub] = 2.0 ** -100
    b_q[p_sub] = b[p_sub] * f32(2.0 ** -35)
    a_q[i_inf, p_inf] = np.inf
    b_q[p_inf, 11] = 0.0
    s_q = chain(a_q, b_q)
    blk = block("relu classes from the product", a_q, b_q, s_q, -1.0, act=RELU)
    blk.reaches = lambda w: _relu_classes(-s_q, w)
    blocks.append(blk)

    # overflow inside the epilogue: fl(alpha s) = +-inf where s is finite; C (beta = 1) holds the opposite infinity on every 7th of
    # those elements, the bias holds +inf on every 5th column and -inf on every 5th + 1: NaN exactly where opposite infinities meet
    big = 3e38
    with np.errstate(over="ignore"):
        r1 = f32(big) * s
    over = np.isinf(r1)
    c_o = c0.copy()
    pick = np.zeros(m * n, bool)
    pick[np.flatnonzero(over.ravel())[::7]] = True
    pick = pick.reshape(m, n)
    c_o[pick] = -r1[pick]
    bias_o = bias_n.copy()
    bias_o[0::5], bias_o[1::5] = np.inf, -np.inf
    blk = block("overflow in the epilogue", a, b, s, big, beta=1.0, c=c_o, bias=bias_o, mode=COL)

    def reaches(w):
        assert over.sum() > s.size // 2 and (r1[over] > 0).any() and (r1[over] < 0).any()
        r2_inf = np.isinf(r1) | np.isinf(bias_o)[None, :]
        nan = pick | (over & np.isinf(bias_o)[None, :] & (np.sign(r1) != np.sign(bias_o)[None, :]))
        assert pick.sum() > 0 and (nan & ~pick).sum() > 0
        assert np.array_equal(np.isnan(w), nan)
        assert np.isinf(w[r2_inf & ~nan]).all() and np.isinf(w[over & ~nan]).sum() > 0
    blk.reaches = reaches
    blocks.append(blk)

    # subnormal beta c beside alpha s of its size: fl(beta c) rounds (a subnormal keeps fewer bits than c has), then the sum
    # rounds -- not the one rounding of fma(beta, c, r1)
    alpha_t, beta_t = 2.0 ** -126, 2.0 ** -10
    c_t = (c0 * f32(2.0 ** -120)).astype(f32)
    blk = block("subnormal beta c", a, b, s, alpha_t, beta=beta_t, c=c_t)

    def reaches(w):
        bc = f32(beta_t) * c_t
        r1_t = f32(alpha_t) * s
        assert _is_subnormal(bc).sum() > s.size // 2 and _is_subnormal(r1_t).sum() > 0 and (np.abs(r1_t) >= TINY).sum() > 0
        assert (bc.astype(np.float64) != np.float64(beta_t) * c_t.astype(np.float64)).sum() > s.size // 4   # the product rounded
        assert (r1_t.astype(np.float64) != np.float64(alpha_t) * s.astype(np.float64)).sum() > 0
        # fma(beta, c, r1): exact in fp64, rounded once.  It differs from the two roundings only where the sum is normal (subnormals
        # add exactly) and fl(beta c) lands on a tie of the sum's coarser grid: one to three bits coarser here, so 1/4 .. 1/16 of
        # the elements with a normal sum -- a few percent of all
        fused = (np.float64(beta_t) * c_t.astype(np.float64) + r1_t.astype(np.float64)).astype(f32)
        assert (fused != w).sum() > s.size // 64
        assert _is_subnormal(w).sum() > 0
    blk.reaches = reaches
    blocks.append(blk)
    return blocks


def _assert(ok):
    assert ok


def _relu_classes(pre, want):
    """`pre`, the value in front of ReLU, takes every class, and `want` is what the contract makes of each."""
    nan, ninf, pinf = np.isnan(pre), np.isneginf(pre), np.isposinf(pre)
    with np.errstate(invalid="ignore"):
        nsub, psub, nz = _is_subnormal(pre) & (pre < 0), _is_subnormal(pre) & (pre > 0), _neg_zero(pre)
    for name, cls in (("NaN", nan), ("-inf", ninf), ("+inf", pinf), ("negative subnormal", nsub), ("positive subnormal", psub), ("-0", nz)):
        assert cls.sum() > 0, f"no {name} in front of ReLU"
    assert np.array_equal(np.isnan(want), nan)
    assert _pos_zero(want[ninf | nsub | nz]).all()
    assert np.isposinf(want[pinf]).all()
    assert np.array_equal(want[psub].view(np.uint32), pre[psub].view(np.uint32)) and _is_subnormal(want[psub]).all()


SPECIAL_TILES = ("mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5")


def special_shapes(kernel, cus):
    """(m, n, k, guarded, stream-K) of a kernel's special-value runs: _special_shapes' whole-tile shape and guarded one with a K
    tail, and on a tile the first guarded ragged stream-K shape of its rows."""
    out = [(m, n, k, guarded, False) for m, n, k, guarded in _special_shapes(kernel)]
    if kernel != "naive":
        bm, bn = (int(x) for x in re.search(r"_(\d+)x(\d+)", kernel).groups())
        m, n, k, _ = _streamk_shapes(bm, bn, True, False)(cus)[0]
        out.append((m, n, k, True, True))
    return out


SPECIAL_CASES = [(kernel, ops) for kernel in ("naive",) + SPECIAL_TILES for ops in EX_OPS.values()]


@pytest.mark.parametrize("kernel,ops", SPECIAL_CASES, ids=[f"{k}_{pair_name(o)}" for k, o in SPECIAL_CASES])
def test_special_values_follow_the_epilogue_contract(mm, oracle, cus, kernel, ops):
    """alpha == 0, signed zeros through switched-off operations, beta == -0, every class of value through ReLU, overflow inside
    the epilogue and a subnormal beta c (special_blocks), bit for bit against numpy: on the naive kernel and on every tile, whole,
    guarded with a K tail, and guarded chained stream-K.  Every block runs; the message lists all that differ."""
    failures = []
    for m, n, k, guarded, sk in special_shapes(kernel, cus):
        with _ExOptions(mm, kernel, 2 if sk else 0, 0):
            for blk in special_blocks(oracle, m, n, k):
                blk.check_expectation()
                got, untouched, launched = run_ex(mm, ops, blk.a, blk.b, blk.alpha, blk.beta, dev(blk.c) if blk.beta != 0 else None,
                                                  blk.bias, blk.mode, blk.act, guarded)
                got = got.cpu().numpy()
                where = (kernel, pair_name(ops), (m, n, k), blk.name)
                tag = ex_tag(ops, blk.alpha, blk.beta, blk.mode, blk.act)
                if kernel == "naive":
                    check_launch(launched, "sgemm_naive_ex_kernel", (), (), tag, where)
                else:
                    bm_bn = re.search(r"_(\d+)x(\d+)", kernel).expand(r"<\1,\2>")
                    words = (["guarded"] if guarded else []) + (["persistent", "chained parts"] if sk else [])
                    check_launch(launched, ("sgemm_dma5_ex_streamk_kernel" if sk else "sgemm_mfma_dma5_ex_kernel") + bm_bn, words,
                                 [w for w in ("guarded", "persistent", "chained parts") if w not in words], tag, where)
                assert untouched, (where, "wrote outside C's window", launched)
                if not same_bits(got, blk.want):
                    failures.append(f"{(m, n, k)} {blk.name}: {first_difference(got, blk.want)}  [{launched}]")
    assert not failures, "\n".join(failures)
    assert mm.streamk_timeouts() == 0
