"""Every LDS-DMA fp32 GEMM instantiation of libmmult_hip.so against the oracle's fused chain, bit for bit.

INSTANTIATIONS has one row per instantiation of the eight LDS-DMA families -- K2L (sgemm_dma.hpp) plain and stream-K, K2W
(sgemm_dma5.hpp) plain and stream-K, K1W (sgemm_valu_dma5.hpp) plain and stream-K, and the transposed-operand forms of
K2W (launch_op.hip) plain and stream-K.  A row says how a caller reaches its instantiation through the C ABI (forced
kernel, MMH_OPT_STREAMK, MMH_OPT_STREAMK_CHAIN, MMH_OPT_PERSIST, operand layouts), which words of mmh_last_launch prove
that it ran, and the shapes it runs.  tests/test_lds_dma_coverage.py holds the table to the symbols of the built library on
the CPU, so a new instantiation cannot ship without a row.

"Bit for bit" is same_bits (tests/bitcmp.py): the uint32 patterns are equal wherever the oracle's value is not NaN (so -0.0 is
not +0.0), and NaN stands where the oracle has NaN (payloads are not compared)."""
import dataclasses
import math
import re
from typing import Callable, Optional

import numpy as np
import pytest

from bitcmp import first_difference, same_bits
from gpu_operands import _Options, _case, cus_fixture, run_gemm
from kernel_tables import (K2L_TILES, K2W_SK, K2W_TILES, OP_LAYOUTS, _plain_shapes, _signed_zero_inputs, _special_shapes,
                           _streamk_shapes)

pytestmark = pytest.mark.gpu
cus = cus_fixture("mm")


# ---- the table --------------------------------------------------------------------------------------------------------
# The K1W tile configurations (launch_valu.hip), spelled as tools/kernel_resources.py demangles them; the K2L and K2W ones:
# tests/kernel_tables.py.
K1W = ("128,128,2,2,2,2,3", "128,64,3,2,2,2,3", "64,64,3,2,2,2,5", "64,64,3,2,2,4,5")
K1W_SK = ("128,128,2,2,2,2", "128,64,3,2,2,3", "64,64,3,2,2,5")
BOOL = ("false", "true")


def _symbols():
    for t in K2L_TILES:
        for e in BOOL:
            yield f"sgemm_mfma_dma_kernel<{t},{e}>"
            yield f"sgemm_dma_streamk_kernel<{t},{e}>"
    for t, nl_d in K2W_TILES.items():
        for e in BOOL:
            yield f"sgemm_mfma_dma5_kernel<{t},{e},{nl_d},1>"
            if t in K2W_SK:
                for chain in BOOL:
                    yield f"sgemm_dma5_streamk_kernel<{t},{e},{chain},{nl_d},1>"
                for op in (1, 2, 3):
                    yield f"sgemm_mfma_dma5_op_kernel<{t},{e},{nl_d},{op}>"
                    yield f"sgemm_dma5_op_streamk_kernel<{t},{e},{nl_d},{op}>"
    for t in K1W:
        yield f"sgemm_valu_dma5_kernel<{t}>"
    for t in K1W_SK:
        yield f"sgemm_valu_dma5_streamk_kernel<{t}>"


# family -> the template arguments after <BM,BN, (named groups: what the reach depends on)
FAMILIES = {
    "sgemm_mfma_dma_kernel": r"32,\d+,\d+,3,(?P<edge>true|false)",
    "sgemm_dma_streamk_kernel": r"32,\d+,\d+,3,(?P<edge>true|false)",
    "sgemm_mfma_dma5_kernel": r"32,\d+,\d+,3,(?P<edge>true|false),\d+,2,1",
    "sgemm_dma5_streamk_kernel": r"32,\d+,\d+,3,(?P<edge>true|false),(?P<chain>true|false),\d+,2,1",
    "sgemm_mfma_dma5_op_kernel": r"32,\d+,\d+,3,(?P<edge>true|false),\d+,2,(?P<op>[123])",
    "sgemm_dma5_op_streamk_kernel": r"32,\d+,\d+,3,(?P<edge>true|false),\d+,2,(?P<op>[123])",
    "sgemm_valu_dma5_kernel": r"\d+,\d+,\d+,(?P<ak>\d+),\d+",
    "sgemm_valu_dma5_streamk_kernel": r"\d+,\d+,\d+,\d+",
}
FAMILY_RE = re.compile(r"^(?P<family>" + "|".join(FAMILIES) + r")<(?P<bm>\d+),(?P<bn>\d+),(?P<rest>.*)>$")


@dataclasses.dataclass(frozen=True)
class Inst:
    symbol: str
    kernel: str                       # forced kernel (MMult.set_kernel)
    streamk: int                      # MMH_OPT_STREAMK: 0 = plain launches only, 2 = stream-K whenever the count is ragged
    chain: int                        # MMH_OPT_STREAMK_CHAIN
    persist: int                      # MMH_OPT_PERSIST
    ops: Optional[tuple]              # (transa, transb) for mmh_sgemm_op; None: mmh_sgemm
    markers: tuple                    # words of mmh_last_launch that must appear ...
    absent: tuple                     # ... and must not
    shapes: Callable                  # cus -> [(m, n, k, whole_rounds)]
    tiles_ok: Optional[Callable] = None   # (tiles, cus) -> bool: which of two instantiations a launch string cannot tell apart

    @property
    def bm_bn(self):
        m = FAMILY_RE.match(self.symbol)
        return int(m["bm"]), int(m["bn"])


def _k1w_shapes(bm, bn, ak):
    def shapes(cus):
        r = math.isqrt(cus) + 1
        if bm == 64 and ak == 2:                               # one CU's worth of tiles or fewer: A read two k-steps at a time
            base = [(64, 64, 32), (256, 192, 96), (512, 1024, 256)]
        elif bm == 64:                                         # more: four
            base = [(r * 64, r * 64, 64), ((r + 1) * 64, r * 64, 160)]
        else:
            base = [(bm, bn, 32), (2 * bm, 3 * bn, 96), (r * bm, 2 * bn, 64)]
        return [(m, n, k, False) for m, n, k in base]
    return shapes


def _row(symbol):
    m = FAMILY_RE.match(symbol)
    assert m, symbol
    fam, bm, bn = m["family"], int(m["bm"]), int(m["bn"])
    g = re.fullmatch(FAMILIES[fam], m["rest"])
    assert g, symbol
    g = g.groupdict()
    edge = g.get("edge") == "true"
    sk = "streamk" in fam
    head = f"{fam}<{bm},{bn}>"
    markers, absent = [head], []
    if "edge" in g:
        (markers if edge else absent).append("guarded")
    if sk:
        markers.append("persistent")
    else:
        absent.append("persistent")
    chain = 1
    if g.get("chain") == "false":
        chain = 0
        absent.append("chained parts")
    elif fam in ("sgemm_dma5_streamk_kernel", "sgemm_dma5_op_streamk_kernel", "sgemm_valu_dma5_streamk_kernel"):
        markers.append("chained parts")
    ops = None
    if "op" in g:
        ops = OP_LAYOUTS[int(g["op"])]
        markers.append("operands " + "NT"[ops[0]] + "NT"[ops[1]])
    tiles_ok = None
    if fam.startswith("sgemm_valu"):
        kernel = f"valu_{bm}x{bn}"
        shapes = _streamk_shapes(bm, bn, False, True) if sk else _k1w_shapes(bm, bn, int(g["ak"]))
        if not sk and bm == 64:
            tiles_ok = (lambda t, cus: t <= cus) if g["ak"] == "2" else (lambda t, cus: t > cus)
        elif not sk and bn == 128:
            tiles_ok = lambda t, cus: t < 4 * cus               # (from four tiles per CU the register-staged K1 runs)
    else:
        kernel = f"mfma_{bm}x{bn}_dma" + ("5" if "dma5" in fam else "")
        shapes = _streamk_shapes(bm, bn, edge, True) if sk else _plain_shapes(bm, bn, edge)
    return Inst(symbol=symbol, kernel=kernel, streamk=2 if sk else 0, chain=chain, persist=1 if sk else 0, ops=ops,
                markers=tuple(markers), absent=tuple(absent), shapes=shapes, tiles_ok=tiles_ok)


def _order(inst):   # rows that run the same shapes next to each other: their inputs and oracle results are reused
    bm, bn = inst.bm_bn
    return (bm, bn, "guarded" in inst.markers, inst.streamk, inst.symbol)


INSTANTIATIONS = sorted((_row(s) for s in _symbols()), key=_order)


# ---- running a row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=lambda i: i.symbol)
def test_every_lds_dma_instantiation_returns_the_oracle_bits(mm, cus, inst):
    guarded = "guarded" in inst.markers
    bm, bn = inst.bm_bn
    with _Options(mm, inst):
        for m, n, k, whole_rounds in inst.shapes(cus):
            tiles = -(-m // bm) * -(-n // bn)
            if inst.tiles_ok is not None:
                assert inst.tiles_ok(tiles, cus), ("shape does not reach the row's instantiation", m, n, k, tiles, cus)
            a, b, c0, want, want_acc = _case(m, n, k)
            for accumulate in (False, True):
                where = (inst.symbol, (m, n, k), "accumulate" if accumulate else "overwrite")
                got, untouched, launched = run_gemm(mm, a, b, c0 if accumulate else None, accumulate, guarded, inst.ops)
                for word in inst.markers:
                    assert word in launched, (where, word, launched)
                for word in inst.absent:
                    assert word not in launched, (where, word, launched)
                if inst.streamk:
                    t, g = (int(x) for x in re.search(r"(\d+) tiles on (\d+) persistent", launched).groups())
                    assert t == tiles
                    assert (t % g == 0 and t >= 2 * g) if whole_rounds else t % g != 0, (where, launched)
                assert untouched, (where, "wrote outside C's window", launched)
                ref = want_acc if accumulate else want
                assert same_bits(got, ref), (where, first_difference(got, ref), launched)
    assert mm.streamk_timeouts() == 0


# ---- special values ---------------------------------------------------------------------------------------------------
SPECIAL_KERNELS = [(f"mfma_{t}_dma", None) for t in ("64x64", "128x64", "128x128")] + \
    [(f"mfma_{t}_dma5", None) for t in ("64x64", "128x64", "128x128", "96x96", "96x64", "160x160")] + \
    [(f"valu_{t}", None) for t in ("64x64", "128x64", "128x128")] + [("naive", None), ("auto", None)] + \
    [(k, None) for k in ("mfma", "mfma_64x64", "mfma_128x64", "mfma_256x256")] + \
    [(f"mfma_{t}_dma5", ops) for t in ("64x64", "128x64", "128x128") for ops in ((0, 1), (1, 0), (1, 1))]


@pytest.mark.parametrize("kernel,ops", SPECIAL_KERNELS,
                         ids=[k + ("" if o is None else "_" + "NT"[o[0]] + "NT"[o[1]]) for k, o in SPECIAL_KERNELS])
def test_special_values_follow_the_chain_on_the_lds_dma_tiles(mm, oracle, kernel, ops):
    """Subnormal products and sums (not flushed; products that underflow to -0 included), overflow to inf at the same
    partial sum, planted inf / NaN (inf * 0 and NaN give NaN in the same elements), and signed zeros: accumulate onto -0
    with every product -0 stays -0, overwrite with every product -0 is +0 -- on a whole-tile shape and on a guarded one
    with a K tail, where the dead k-lanes of the last K-step take part in the MFMA.  (valu_* run K1W on the whole shape
    and K1's register-staged guarded kernel on the other; mfma* are the register-staged K2 tiles, which share that
    kernel's guarded loader.)"""
    mm.set_kernel(kernel)
    failures = []   # every block on both shapes runs: which of them differ is the finding
    try:
        for m, n, k, guarded in _special_shapes(kernel):
            a, b = oracle.harness_inputs(m, n, k, seed=99 + k)
            blocks = []
            blocks.append(("subnormal", (a * np.float32(1e-21)).astype(np.float32), (b * np.float32(1e-21)).astype(np.float32), None))
            blocks.append(("overflow", (a * np.float32(3e19)).astype(np.float32), (b * np.float32(3e19)).astype(np.float32), None))
            a_p, b_p = a.copy(), b.copy()
            a_p[3, 5], a_p[70, 10], b_p[5, 7], b_p[20, 100] = np.inf, -np.inf, 0.0, np.nan
            blocks.append(("inf/nan", a_p, b_p, None))
            a_z, b_z, c_z, neg_zero = _signed_zero_inputs(a, b)
            blocks.append(("signed zero, overwrite", a_z, b_z, None))
            blocks.append(("signed zero, accumulate", a_z, b_z, c_z))
            for name, x, y, c in blocks:
                with np.errstate(over="ignore", invalid="ignore"):
                    want = oracle.ref_mmult(x, y, None if c is None else c.copy(), fma=True)
                if name == "subnormal":
                    assert np.any((want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)), "must reach subnormals"
                elif name == "overflow":
                    assert np.isinf(want).any()
                elif name == "inf/nan":
                    assert np.isnan(want[3, 7]) and np.isnan(want[:, 100]).all() and np.isinf(want[70]).any()
                elif name == "signed zero, overwrite":
                    assert (want[neg_zero] == 0).all() and not np.signbit(want[neg_zero]).any()
                else:
                    assert (want[neg_zero] == 0).all() and np.signbit(want[neg_zero]).all()
                got, untouched, launched = run_gemm(mm, x, y, c, c is not None, guarded, ops)
                where = (kernel, ops, (m, n, k), name, launched)
                assert untouched, where
                if ops is not None:
                    assert "operands " + "NT"[ops[0]] + "NT"[ops[1]] in launched, where
                elif "_dma" in kernel:
                    assert "LDS-DMA" in launched and ("guarded" in launched) == guarded, where
                if not same_bits(got, want):
                    failures.append(f"{(m, n, k)} {name}: {first_difference(got, want)}  [{launched}]")
        assert not failures, "\n".join(failures)
    finally:
        mm.set_kernel("mfma")


# ---- AUTO where it picks the odd-blocked K2W tiles --------------------------------------------------------------------
AUTO_SHAPES = [(2560, 2560, 2560), (1152, 1152, 1152), (2603, 2344, 1132), (3554, 1499, 176), (2673, 476, 1736), (2037, 688, 1286)]


@pytest.mark.parametrize("m,n,k", AUTO_SHAPES)
def test_auto_on_the_96x64_and_160x160_tiles_returns_the_oracle_bits(mm, oracle, cus, m, n, k):
    import torch
    import how_to_optimize_gemm_amd as H
    name, _, _ = H.auto_plan(m, n, k, cu_count=cus)
    assert name in ("mfma_96x64_dma5", "mfma_160x160_dma5"), (m, n, k, name)
    tile = "<" + name.split("_")[1].replace("x", ",") + ">"
    a, b = oracle.harness_inputs(m, n, k, seed=m ^ n ^ k)
    c0 = np.random.default_rng(k).uniform(-1, 1, (m, n)).astype(np.float32)
    mm.set_kernel("auto")
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got = mm.matmul(da, db)
    assert tile in H.last_launch(), (name, H.last_launch())
    want = oracle.ref_mmult(a, b, fma=True)
    assert same_bits(got.cpu().numpy(), want), first_difference(got.cpu().numpy(), want)
    out = torch.from_numpy(c0).cuda()
    mm.matmul(da, db, out=out, accumulate=True)
    assert tile in H.last_launch(), (name, H.last_launch())
    want = oracle.ref_mmult(a, b, c0.copy(), fma=True)
    assert same_bits(out.cpu().numpy(), want), first_difference(out.cpu().numpy(), want)
    mm.set_kernel("mfma")
