"""Every instantiation of the register-staged K1 kernel (csrc/sgemm_valu.hpp sgemm_valu_kernel, launched from
csrc/launch_valu.hip) against the oracle's fused chain, bit for bit, overwrite and accumulate.

Since K1W (sgemm_valu_dma5_*) took the whole-tile shapes, the two whole-tile instantiations of K1 run only where K1W does
not: beyond the buffer-descriptor window (launch_valu_w returns 1 and launch_valu_tile picks `fast` by the tile's own K-slice
depth), and, for the 128x128 tile, from four tiles per CU.  K1_INSTANTIATIONS has one row per instantiation, in the style of
tests/test_gpu_reg_parity.py::REG_INSTANTIATIONS (tests/gpu_operands.py runs the rows of both): a row says which forced kernels reach its
instantiation, which words of mmh_last_launch prove it, and the shapes it runs.  tests/test_k1_coverage.py holds the table to
the symbols of the built library on the CPU and proves every case's route on launch_valu.hip's host arithmetic, restated in
`k1_route` below.

The kernel keeps ONE K-slice in LDS and parks the next one in registers (NBUF = 1): one slice (no load in the loop), two
(one parked slice, no steady state) and three or more are different paths through it, and the rows run all three."""
import dataclasses
import math
import re

import pytest

from bitcmp import first_difference, same_bits
from gpu_operands import BIG_FLOATS, _case, _ld, _reach, big, cus_fixture, run_strided   # noqa: F401 (big: a fixture)
from kernel_tables import _edge_cases, smallest_beyond, window_ok

pytestmark = pytest.mark.gpu
cus = cus_fixture("mm")

K1_HEAD = "sgemm_valu_kernel"
K1W_HEAD = "sgemm_valu_dma5"
# BM, BN -> the K-slice depth and the fragment look-ahead launch_valu_tile instantiates the tile with
K1_TILES = {(64, 64): (64, 4), (128, 128): (32, 1)}
# BM, BN -> the forced kernels whose launcher ends in launch_valu_tile<BM, BN> (valu_128x64 has no K1 tile of its own: its guarded
# shapes run the 128x128 one; a whole-tile row runs on its tile's own id, whose window its leading dimensions are sized for)
K1_KERNELS = {(64, 64): ("valu_64x64",), (128, 128): ("valu_128x128", "valu_128x64")}
FAMILY_RE = re.compile(r"^sgemm_valu_kernel<(?P<bm>\d+),(?P<bn>\d+),(?P<kb>\d+),(?P<edge>true|false),1,(?P<p>\d+)>$")


@dataclasses.dataclass(frozen=True)
class K1Case:
    m: int
    n: int
    k: int
    lda: int = 0                 # 0: run_gemm's small padded leading dimension; else A is a view of the NaN buffer
    ldb: int = 0                 # likewise B
    aligned: bool = True         # leading dimensions multiples of 4 and 16-byte bases (False: odd and 4 bytes past)
    kernels: tuple = ()          # the forced kernels that run the case (empty: every one of the row)
    production: bool = False     # the route N = 4096 takes: the window holds, four tiles per CU or more


@dataclasses.dataclass(frozen=True)
class K1:
    symbol: str
    bm: int
    bn: int
    kb: int
    guarded: bool
    kernels: tuple

    @property
    def markers(self):
        return (f"{K1_HEAD}<{self.bm},{self.bn}>",) + (("guarded",) if self.guarded else ())

    @property
    def absent(self):
        return (K1W_HEAD,) + (() if self.guarded else ("guarded",))

    def cases(self, cus):
        bm, bn, kb = self.bm, self.bn, self.kb
        if self.guarded:
            # tails 0, 1 and KB - 1, a tail behind two and more slices, m and n below the tile, several ragged tiles, odd leading
            # dimensions and 4-byte bases (the register-staged table's shapes for this tile's own slice depth)
            out = [K1Case(c.m, c.n, c.k, aligned=False) for c in _edge_cases(bm, bn, kb)]
            if kb > 32:
                # whole tiles, aligned operands, k a multiple of 32 but not of the tile's slice: K1W's rule (32-deep slices) takes
                # the shape, the window sends it back, and only `fast` by the tile's OWN depth keeps it off the whole-tile kernel
                k = kb + 32
                out.append(K1Case(bm, bn, k, ldb=smallest_beyond("b", bm, bn, k, False)))
            return out
        # by the window: one tile, one K-slice, B then A beyond it
        out = [K1Case(bm, bn, kb, ldb=smallest_beyond("b", bm, bn, kb, False)), K1Case(bm, bn, kb, lda=smallest_beyond("a", bm, bn, kb, False))]
        # by pipeline depth: two slices (one parked, no steady state) and seven, 2 x 3 tiles (block_to_tile)
        out += [K1Case(2 * bm, 3 * bn, nk * kb, ldb=smallest_beyond("b", bm, bn, nk * kb, False)) for nk in (2, 7)]
        if (bm, bn) == (128, 128):
            # by the production route: tiles >= 4 CUs keeps the shape off K1W with every operand inside the window
            side = 128 * math.ceil(math.sqrt(4 * cus))
            out.append(K1Case(side, side, 64, kernels=("valu_128x128",), production=True))
        return out

    def leading_dimensions(self, case):
        guarded = not case.aligned
        return case.lda or _ld(case.k, guarded), case.ldb or _ld(case.n, guarded), _ld(case.n, guarded)


def _table_rows():
    for (bm, bn), (kb, p) in K1_TILES.items():
        for edge in ("false", "true"):
            yield K1(symbol=f"{K1_HEAD}<{bm},{bn},{kb},{edge},1,{p}>", bm=bm, bn=bn, kb=kb, guarded=edge == "true",
                     kernels=K1_KERNELS[(bm, bn)] if edge == "true" else K1_KERNELS[(bm, bn)][:1])


K1_INSTANTIATIONS = list(_table_rows())


def k1_route(kernel, case, lds, cus, streamk=0):
    """csrc/launch_valu.hip restated for a forced valu_* id with stream-K off: (family, BM, BN, guarded) of the kernel that runs.
    launch_valu_w takes whole 32-deep shapes (fast_shape(BM, BN, 32)) inside the window (window_ok) -- the 128x128 tile only
    below four tiles per CU --; launch_valu_tile<BM, BN, KB> everything else, `fast` by fast_shape(BM, BN, KB)."""
    assert streamk == 0, "launch_valu_sk comes first with stream-K on"
    lda, ldb, ldc = lds
    aligned = case.aligned and lda % 4 == 0 and ldb % 4 == 0 and ldc % 4 == 0

    def fast(bm, bn, kb):
        return aligned and case.m % bm == 0 and case.n % bn == 0 and case.k % kb == 0

    def w(bm, bn):
        return fast(bm, bn, 32) and window_ok(bm, bn, case.k, lda, ldb)

    def k1(bm, bn):
        return (K1_HEAD, bm, bn, not fast(bm, bn, K1_TILES[(bm, bn)][0]))

    def k1_128():
        tiles = math.ceil(case.m / 128) * math.ceil(case.n / 128)
        return (K1W_HEAD, 128, 128, False) if tiles < 4 * cus and w(128, 128) else k1(128, 128)

    if kernel == "valu_64x64":
        return (K1W_HEAD, 64, 64, False) if w(64, 64) else k1(64, 64)
    if kernel == "valu_128x64":
        return (K1W_HEAD, 128, 64, False) if w(128, 64) else k1_128()
    assert kernel == "valu_128x128", kernel
    return k1_128()


@pytest.mark.parametrize("row", K1_INSTANTIATIONS, ids=lambda r: r.symbol)
def test_every_k1_instantiation_returns_the_oracle_bits(mm, cus, big, row):
    for kernel in row.kernels:
        with _reach(mm, kernel, streamk=0):   # (its exit restores the kernel and the stream-K option, whatever happens)
            for case in row.cases(cus):
                if case.kernels and kernel not in case.kernels:
                    continue
                assert k1_route(kernel, case, row.leading_dimensions(case), cus) == (K1_HEAD, row.bm, row.bn, row.guarded), \
                    ("shape does not reach the row's instantiation", kernel, case)
                a, b, c0, want, want_acc = _case(case.m, case.n, case.k)
                for accumulate in (False, True):
                    where = (row.symbol, kernel, case, "accumulate" if accumulate else "overwrite")
                    got, untouched, launched = run_strided(mm, big, a, b, c0 if accumulate else None, accumulate, not case.aligned,
                                                           case.lda, case.ldb)
                    print(where, launched)
                    for word in row.markers:
                        assert word in launched, (where, word, launched)
                    for word in row.absent:
                        assert word not in launched, (where, word, launched)
                    assert untouched, (where, "wrote outside C's window", launched)   # (an operand beyond the window: NaN all around it)
                    ref = want_acc if accumulate else want
                    assert same_bits(got, ref), (where, first_difference(got, ref), launched)
