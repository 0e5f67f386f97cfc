"""Every fused-epilogue instantiation of libmmult_hip.so (mmh_sgemm_ex: sgemm_mfma_dma5_ex_kernel and
sgemm_dma5_ex_streamk_kernel, csrc/sgemm_dma5.hpp EP, csrc/launch_ex.hip, csrc/launch_ex_t.hip) against the numpy expectation
of the contract, bit for bit, and the special values of the epilogue on every tile and on the naive kernel.

EX_INSTANTIATIONS has one row per instantiation: three tiles x whole / guarded x plain / chained stream-K x four operand
pairs = 48.  A row says how a caller reaches it (forced kernel, MMH_OPT_STREAMK, MMH_OPT_PERSIST, operand pair), which words
of mmh_last_launch prove that it ran, and the shapes it runs -- the ones the NN and op rows of the same tile and edge run in
tests/test_gpu_lds_dma_parity.py.  tests/test_ex_coverage.py holds the table to the symbols of the built library on the CPU.

The expectation is tests/ex_ref.py's `expected` on the oracle's fused chain: numpy alone.  sgemm_naive_ex_kernel calls
the tiles' dma5_epilogue_apply, so for the epilogue it is no independent reference; numpy is the only one."""
import dataclasses
import functools
import re
from typing import Callable

import numpy as np
import pytest

from bitcmp import first_difference, same_bits, same_bits_on_device
from ex_ref import COL, NONE, RELU, ROW, expected
from gpu_operands import _case, _ld, _padded, cus_fixture, dev
from kernel_tables import (K2W_SK, K2W_TILES, OP_LAYOUTS, _plain_shapes, _special_shapes, _streamk_shapes, ex_tag, pair_name,
                           special_blocks)

pytestmark = pytest.mark.gpu
cus = cus_fixture("mm")

# ---- the table --------------------------------------------------------------------------------------------------------
EX_OPS = {0: (0, 0), **OP_LAYOUTS}   # the OP template argument = transa | transb << 1 -> (transa, transb)
EX_FAMILY_RE = re.compile(r"^(?P<family>sgemm_mfma_dma5_ex_kernel|sgemm_dma5_ex_streamk_kernel)<(?P<bm>\d+),(?P<bn>\d+),32,\d+,\d+,3,"
                          r"(?P<edge>true|false),\d+,2,(?P<op>[0-3])>$")


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
# (the blocks: special_blocks, tests/kernel_tables.py)
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
