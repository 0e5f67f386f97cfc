"""Every register-staged MFMA instantiation of libmmult_hip.so (csrc/sgemm_mfma.hpp, launched from csrc/launch_reg.hip) against
the oracle's fused chain, bit for bit -- and the addressing beyond, at the edge of and far past the 2 GiB buffer-descriptor
window.

REG_INSTANTIATIONS has one row per instantiation of sgemm_mfma_kernel, sgemm_mfma_streamk_kernel and sgemm_mfma_simple_kernel,
in the style of tests/test_gpu_lds_dma_parity.py::INSTANTIATIONS (tests/gpu_operands.py runs the rows of both); the opt-in split-K
instantiations, which are not chain kernels, have a table and a bit contract of their own (tests/test_gpu_splitk_parity.py).
A row says how a caller reaches its instantiation through the C ABI -- forced kernel, MMH_OPT_STREAMK, MMH_OPT_PERSIST, whole
or guarded operands, each operand inside or beyond the descriptor window --, which words of mmh_last_launch prove that its
family and form ran, and the shapes it runs.  The launch string does not say whether the descriptor (BUFLD) or the 64-bit
instantiation ran: that is a pure function of (BM, BN, k, lda, ldb), window_ok below (csrc/internal.hpp restated), asserted
for every shape a row runs.  tests/test_reg_coverage.py holds the table to the symbols of the built library on the CPU.

An operand beyond the window spans 2.0 - 2.2 GiB of address space of which only k (A) or n (B) columns per row are written: it
is a strided view into one module-wide NaN buffer, and NaN goes back over what was written when the case ends."""
import dataclasses
import math
import re
from typing import Callable, Optional

import numpy as np
import pytest

from bitcmp import first_difference, same_bits
from gpu_operands import BIG_FLOATS, _case, _ld, _reach, _strided, big, cus_fixture, run_strided   # noqa: F401 (big: a fixture)
from kernel_tables import LIM, REG_TILES, Case, _edge_cases, _parity, per_cu_by_lds, smallest_beyond, window_ok

pytestmark = pytest.mark.gpu
cus = cus_fixture("mm")

FAR_LD = 1 << 20                # lda = ldc of the operands past 4 GiB


def largest_inside(side, bm, bn, k, guarded) -> int:
    """The largest lda (side "a") / ldb ("b") window_ok admits for the tile: odd for a guarded shape, a multiple of 4 for a whole one."""
    q = LIM // 4 - 1
    ld = (q - k) // bm if side == "a" else (q - bn) // k
    while not _parity(ld, guarded):
        ld -= 1
    return ld


def past_2_31(rows) -> int:
    """The smallest leading dimension, a multiple of 4, that puts the last of `rows` rows at a byte offset of 2^31 or more."""
    ld = -(-(1 << 29) // (rows - 1))
    return ld + (-ld) % 4


def fallback_tile(m, n, cus):
    """csrc/policy.hip fallback_kernel: the register-staged tile MMH_KERNEL_AUTO runs when no LDS-DMA family takes the shape."""
    t = lambda bm, bn: -(-m // bm) * -(-n // bn)
    if t(256, 256) >= cus:
        return 256, 256
    if t(128, 64) * 2 <= cus:
        return 64, 64
    if t(128, 128) * 10 < cus * 8:
        return 128, 64
    return 128, 128


# ---- the table --------------------------------------------------------------------------------------------------------
# (REG_TILES, tests/kernel_tables.py: forced kernel -> BM, BN, WTN, WTM, KB)
SK_TILES = ("mfma", "mfma_256x256", "mfma_128x64", "mfma_64x64")     # reg_tiles: the ones with a stream-K form
BEYOND_KERNELS = ("mfma", "mfma256", "mfma_256x256", "mfma_128x64", "mfma_64x64", "mfma_pipe")
BOOL = ("false", "true")
UNREACHABLE = {"sgemm_mfma_kernel<128,128,true,0,0,true,4,4,32,false>":
               "csrc/launch_reg.hip:34 -- launch_mfma<128,128,false,0,0,false> (mfma_pipe) instantiates it in the guarded branch's "
               "`BUFLD && win ? ... : ...`, whose condition folds to false with the template argument BUFLD = false"}


def _symbols():
    for bm, bn, wtn, wtm, kb in REG_TILES.values():
        for e in BOOL:
            for bufld in BOOL:
                yield f"sgemm_mfma_kernel<{bm},{bn},{e},4,0,{bufld},{wtn},{wtm},{kb},false>"
    yield "sgemm_mfma_kernel<128,128,false,0,0,false,4,4,32,false>"      # mfma_pipe: compiler-scheduled, 64-bit addressing always
    yield "sgemm_mfma_kernel<128,128,true,0,0,false,4,4,32,false>"
    yield from UNREACHABLE
    for name in SK_TILES:
        bm, bn, wtn, wtm, kb = REG_TILES[name]
        for e in BOOL:
            yield f"sgemm_mfma_streamk_kernel<{bm},{bn},{e},{wtn},{wtm},{kb}>"
    for e in BOOL:
        yield f"sgemm_mfma_simple_kernel<128,128,{e}>"


# family -> the template arguments after <BM,BN,
FAMILIES = {
    "sgemm_mfma_kernel": r"(?P<edge>true|false),(?P<sched>\d+),0,(?P<bufld>true|false),(?P<wtn>\d+),(?P<wtm>\d+),(?P<kb>\d+),false",
    "sgemm_mfma_streamk_kernel": r"(?P<edge>true|false),(?P<wtn>\d+),(?P<wtm>\d+),(?P<kb>\d+)",
    "sgemm_mfma_simple_kernel": r"(?P<edge>true|false)",
}
FAMILY_RE = re.compile(r"^(?P<family>" + "|".join(FAMILIES) + r")<(?P<bm>\d+),(?P<bn>\d+),(?P<rest>.*)>$")


@dataclasses.dataclass(frozen=True)
class Reg:
    symbol: str
    kernels: tuple = ()               # forced kernels (MMult.set_kernel) that reach the instantiation; every one runs every case
    streamk: int = 0                  # MMH_OPT_STREAMK: 0 = plain launches only, 2 = stream-K whenever the count is ragged
    persist: int = 0                  # MMH_OPT_PERSIST (it applies to this family: launch_common.hpp streamk_wanted)
    guarded: bool = False             # odd leading dimensions and bases 4 bytes past 16-byte alignment
    markers: tuple = ()               # words of mmh_last_launch that must appear ...
    absent: tuple = ()                # ... and must not
    cases: Optional[Callable] = None  # cus -> [Case]
    bufld: Optional[bool] = None      # what window_ok must say of every case (None: the instantiation is not chosen by it)
    unreachable: Optional[str] = None  # file:line and the constant that folds: no call reaches the instantiation

    @property
    def parsed(self):
        m = FAMILY_RE.match(self.symbol)
        return m["family"], int(m["bm"]), int(m["bn"]), re.fullmatch(FAMILIES[m["family"]], m["rest"]).groupdict()

    @property
    def tile(self):                   # BM, BN, KB
        _, bm, bn, g = self.parsed
        return bm, bn, int(g.get("kb", 32))

    def leading_dimensions(self, case):
        return case.lda or _ld(case.k, self.guarded), case.ldb or _ld(case.n, self.guarded)

    def reached_by(self, case) -> bool:
        """Whether launch_mfma's `BUFLD && win` picks this row's instantiation for the case (window_ok, as tiles_ok is used
        in tests/test_gpu_lds_dma_parity.py); the persistent launch needs the window too (try_launch_streamk)."""
        bm, bn, _ = self.tile
        return self.bufld is None or window_ok(bm, bn, case.k, *self.leading_dimensions(case)) == self.bufld


def _whole_cases(bm, bn, kb):
    return [Case(bm, bn, kb), Case(2 * bm, 3 * bn, 7 * kb)]


def _beyond_cases(bm, bn, kb, guarded):
    """An operand beyond the window, B then A: the smallest leading dimension that fails window_ok.  Whole: one tile, one
    K-slice (and the same with the operand's last row at byte offset 2^31).  Guarded: m, n ragged by one tile plus 1 and 17,
    one K-slice plus 1."""
    m, n, k = (bm + 1, bn + 17, kb + 1) if guarded else (bm, bn, kb)
    out = [Case(m, n, k, ldb=smallest_beyond("b", bm, bn, k, guarded)), Case(m, n, k, lda=smallest_beyond("a", bm, bn, k, guarded))]
    if not guarded:
        # window_ok bounds k * ldb and BM * lda, one row more than a tile reaches: at the smallest leading dimension it refuses
        # the last row's byte offset is still below 2^31.  These two put it at 2^31 and past it, where a whole-tile
        # descriptor (extent 0x7fffffff) returns zeros -- the cases that tell the two loaders apart by their results.
        out += [Case(m, n, k, ldb=past_2_31(k)), Case(m, n, k, lda=past_2_31(m))]
    return out


def whole_round_tiles_per_cu(w):
    each = math.lcm(*range(1, w + 1))
    return each * -(-2 * w // each)


def _streamk_cases(bm, bn, kb, guarded):
    """r * r tiles, r = isqrt(cus) + 1: a ragged count above one tile per CU and below two (forced stream-K hands tiles over
    between workgroups); k of three K-slices on the 256x256 tile (the oracle's loop), five on the others.  With
    MMH_OPT_PERSIST a whole number (>= 2) of rounds of every grid the launcher can pick (1 .. w workgroups per CU, w what
    the LDS allows): the smallest multiple of lcm(1 .. w) tiles per CU that is at least 2 w."""
    def cases(cus):
        r = math.isqrt(cus) + 1
        nks = 3 if bm == 256 else 5
        w = per_cu_by_lds(bm, bn, kb)
        rounds = whole_round_tiles_per_cu(w)
        if guarded:
            return [Case((r - 1) * bm + 7, r * bn - 3, nks * kb - 3), Case(rounds * bm - 3, cus * bn - 1, 3 * kb - 3, whole_rounds=True)]
        return [Case(r * bm, r * bn, nks * kb), Case(rounds * bm, cus * bn, 3 * kb, whole_rounds=True)]
    return cases


def _row(symbol):
    m = FAMILY_RE.match(symbol)
    assert m, symbol
    fam, bm, bn = m["family"], int(m["bm"]), int(m["bn"])
    g = re.fullmatch(FAMILIES[fam], m["rest"])
    assert g, symbol
    g = g.groupdict()
    if symbol in UNREACHABLE:
        return Reg(symbol=symbol, unreachable=UNREACHABLE[symbol])
    edge = g["edge"] == "true"
    kb = int(g.get("kb", 32))
    head = f"{fam}<{bm},{bn}>"
    guard_words = ((head, "guarded"), ()) if edge else ((head,), ("guarded",))
    if fam == "sgemm_mfma_simple_kernel":
        cases = _edge_cases(bm, bn, kb) if edge else _whole_cases(bm, bn, kb)
        return Reg(symbol=symbol, kernels=("mfma_simple",), guarded=edge, markers=guard_words[0], absent=guard_words[1] + ("persistent",),
                   cases=lambda cus: cases)
    tile = (bm, bn, int(g["wtn"]), int(g["wtm"]), kb)
    names = [name for name, t in REG_TILES.items() if t == tile]
    assert len(names) == 1, symbol
    if fam == "sgemm_mfma_streamk_kernel":
        return Reg(symbol=symbol, kernels=(names[0],), streamk=2, persist=1, guarded=edge, markers=guard_words[0] + ("persistent",),
                   absent=guard_words[1], cases=_streamk_cases(bm, bn, kb, edge), bufld=True)
    absent = guard_words[1] + ("persistent",)
    inside = _edge_cases(bm, bn, kb) if edge else _whole_cases(bm, bn, kb)
    beyond = _beyond_cases(bm, bn, kb, edge)
    if g["sched"] == "0":    # mfma_pipe: launch_mfma<128,128,false,0,0,false> -- 64-bit addressing inside the window and beyond it
        cases = inside + beyond
        return Reg(symbol=symbol, kernels=("mfma_pipe",), guarded=edge, markers=guard_words[0], absent=absent, cases=lambda cus: cases)
    if g["bufld"] == "true":
        kernels = (names[0], "mfma_tiles") if names[0] == "mfma" else (names[0],)   # mfma_tiles: the 128x128 tile, never stream-K
        return Reg(symbol=symbol, kernels=kernels, guarded=edge, markers=guard_words[0], absent=absent, cases=lambda cus: inside, bufld=True)
    return Reg(symbol=symbol, kernels=(names[0],), guarded=edge, markers=guard_words[0], absent=absent, cases=lambda cus: beyond, bufld=False)


def _order(row):   # rows that run the same shapes next to each other: their inputs and oracle results are reused
    _, bm, bn, _ = row.parsed
    return (bm, bn, row.guarded, row.streamk, row.symbol)


REG_INSTANTIATIONS = sorted((_row(s) for s in _symbols()), key=_order)


# ---- running a row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", REG_INSTANTIATIONS, ids=lambda r: r.symbol)
def test_every_register_staged_instantiation_returns_the_oracle_bits(mm, cus, big, row):
    if row.unreachable is not None:
        return   # nothing to run here: tests/test_reg_coverage.py checks the row's claim
    bm, bn, _ = row.tile
    for kernel in row.kernels:
        with _reach(mm, kernel, row.streamk, row.persist):
            for case in row.cases(cus):
                assert row.reached_by(case), ("shape does not reach the row's instantiation", case)
                m, n, k = case.m, case.n, case.k
                tiles = -(-m // bm) * -(-n // bn)
                a, b, c0, want, want_acc = _case(m, n, k)
                for accumulate in (False, True):
                    where = (row.symbol, kernel, case, "accumulate" if accumulate else "overwrite")
                    got, untouched, launched = run_strided(mm, big, a, b, c0 if accumulate else None, accumulate, row.guarded,
                                                           case.lda, case.ldb)
                    for word in row.markers:
                        assert word in launched, (where, word, launched)
                    for word in row.absent:
                        assert word not in launched, (where, word, launched)
                    if row.streamk:
                        t, g = (int(x) for x in re.search(r"(\d+) tiles on (\d+) persistent", launched).groups())
                        assert t == tiles
                        assert (t % g == 0 and t >= 2 * g) if case.whole_rounds else t % g != 0, (where, launched)
                    assert untouched, (where, "wrote outside C's window", launched)
                    ref = want_acc if accumulate else want
                    assert same_bits(got, ref), (where, first_difference(got, ref), launched)
    assert mm.streamk_timeouts() == 0


# ---- the descriptor paths at the edge of the window ---------------------------------------------------------------------
# kernel -> BM, BN, KB, the register-staged tile its catalogue row falls back to (csrc/abi.hip; None: it is one itself)
BOUNDARY_KERNELS = {"mfma": (128, 128, 32, None), "mfma_64x64": (64, 64, 128, None), "mfma_128x128_dma": (128, 128, 32, (128, 128)),
                    "mfma_128x128_dma5": (128, 128, 32, (128, 128)), "mfma_64x64_dma5": (64, 64, 32, (64, 64))}
FALLBACK_IDS = tuple(k for k, v in BOUNDARY_KERNELS.items() if v[3] is not None)
SMALLEST_DMA_TILE = (64, 64)   # of the LDS-DMA families MMH_KERNEL_AUTO prices (k2l_tiles, k2w_tiles): if its window fails, every family's does


def boundary_shape(kernel, guarded):
    """k = one K-slice plus 1 with m = BM + 1, n = BN + 17 (guarded), or one whole tile of one K-slice."""
    bm, bn, kb, _ = BOUNDARY_KERNELS[kernel]
    return (bm + 1, bn + 17, kb + 1) if guarded else (bm, bn, kb)


def boundary_cases(kernel, step):
    """(guarded, Case) with the largest ldb, then lda, window_ok admits for the kernel's tile -- `step` admissible steps
    further (0: just inside, 1: one step outside)."""
    bm, bn, _, _ = BOUNDARY_KERNELS[kernel]
    out = []
    for guarded in (True, False):
        m, n, k = boundary_shape(kernel, guarded)
        inc = step * (2 if guarded else 4)
        out.append((guarded, Case(m, n, k, ldb=largest_inside("b", bm, bn, k, guarded) + inc)))
        out.append((guarded, Case(m, n, k, lda=largest_inside("a", bm, bn, k, guarded) + inc)))
    return out


def _boundary_window(kernel, guarded, case, tile=None):
    bm, bn, _, _ = BOUNDARY_KERNELS[kernel]
    return window_ok(*(tile or (bm, bn)), case.k, case.lda or _ld(case.k, guarded), case.ldb or _ld(case.n, guarded))


def planned_tile(case, guarded, cus):
    """The tile mmh_auto_plan names for the case as run_strided lays it out."""
    import how_to_optimize_gemm_amd as H
    name, _, _ = H.auto_plan(case.m, case.n, case.k, lda=case.lda or _ld(case.k, guarded), ldb=case.ldb or _ld(case.n, guarded),
                             ldc=_ld(case.n, guarded), base_align=4 if guarded else 16, cu_count=cus)
    t = re.search(r"_(\d+)x(\d+)", name)
    return (int(t[1]), int(t[2])) if t else (128, 128)   # ("mfma": the 128x128 register-staged tile)


def _run_both_ways(mm, big, case, guarded, check):
    a, b, c0, want, want_acc = _case(case.m, case.n, case.k)
    for accumulate in (False, True):
        got, untouched, launched = run_strided(mm, big, a, b, c0 if accumulate else None, accumulate, guarded, case.lda, case.ldb)
        where = (case, "guarded" if guarded else "whole", "accumulate" if accumulate else "overwrite", launched)
        check(launched, where)
        assert untouched, (where, "wrote outside C's window")
        ref = want_acc if accumulate else want
        assert same_bits(got, ref), (where, first_difference(got, ref))


@pytest.mark.parametrize("kernel", list(BOUNDARY_KERNELS))
def test_the_largest_leading_dimension_inside_the_window_runs_the_descriptor_path(mm, big, kernel):
    """The descriptor loaders' 32-bit offsets (sgemm_mfma.hpp ext_a / ext_b, sgemm_tile.hpp buf_offsets, the K2L / K2W pieces)
    are safe only by window_ok's margin: the largest leading dimension it admits, B then A, guarded and whole."""
    bm, bn, _, fallback = BOUNDARY_KERNELS[kernel]

    def check(launched, where):
        if fallback is not None:
            assert "LDS-DMA" in launched, where
        else:
            assert f"sgemm_mfma_kernel<{bm},{bn}>" in launched, where
        assert ("guarded" in launched) == where[1].startswith("guarded"), where
    with _reach(mm, kernel):
        for guarded, case in boundary_cases(kernel, 0):
            assert _boundary_window(kernel, guarded, case)
            assert not _boundary_window(kernel, guarded, dataclasses.replace(
                case, lda=case.lda and case.lda + (2 if guarded else 4), ldb=case.ldb and case.ldb + (2 if guarded else 4)))
            _run_both_ways(mm, big, case, guarded, check)


@pytest.mark.parametrize("kernel", FALLBACK_IDS)
def test_one_step_outside_the_window_a_forced_lds_dma_id_runs_its_fallback_tile(mm, cus, big, kernel):
    """... and MMH_KERNEL_AUTO fallback_kernel's tile, once the window of every LDS-DMA family fails (the 64x64 tiles'; a
    128x128 id's step leaves the smaller families inside, and AUTO on them)."""
    bm, bn, _, fallback = BOUNDARY_KERNELS[kernel]
    for guarded, case in boundary_cases(kernel, 1):
        assert not _boundary_window(kernel, guarded, case)

        def forced(launched, where):
            assert "sgemm_mfma_kernel<%d,%d>" % fallback in launched and "LDS-DMA" not in launched, where
        with _reach(mm, kernel):
            _run_both_ways(mm, big, case, guarded, forced)

        planned = planned_tile(case, guarded, cus)

        def auto(launched, where):
            if _boundary_window(kernel, guarded, case, SMALLEST_DMA_TILE):   # a smaller family still windows the operand
                assert "<%d,%d>" % planned in launched, (where, planned)
            else:
                assert planned == fallback_tile(case.m, case.n, cus), (where, planned)
                assert "sgemm_mfma_kernel<%d,%d>" % planned in launched and "LDS-DMA" not in launched, where
        with _reach(mm, "auto", streamk=1):
            _run_both_ways(mm, big, case, guarded, auto)


# ---- A and C past 4 GiB, every tile inside the window -------------------------------------------------------------------
# kernel -> BM, BN, k (one K-slice plus 1)
FAR_KERNELS = {"mfma": (128, 128, 33), "mfma_256x256": (256, 256, 33), "mfma_64x64": (64, 64, 129), "mfma_128x128_dma": (128, 128, 33),
               "mfma_128x128_dma5": (128, 128, 33), "mfma_64x64_dma5": (64, 64, 33), "auto": (128, 128, 33)}
FAR_STREAMK = ("mfma_64x64_dma5", "mfma_64x64")
# rows in front of the last tile row: from row 1024 on a row of 2^20 floats lies past BYTE offset 2^32 (a 32-bit byte offset
# wraps), from row 2048 on past ELEMENT offset 2^31 (an int product row * ld wraps)
FAR_ROWS = (1024, 2048)
FAR_MAX_ROWS = max(FAR_ROWS) + 256 + 1
FAR_C_COLUMN = 4096             # A is columns 0 .. k of the buffer's rows, C columns 4096 .. 4096 + n of the same rows


def far_shape(kernel, rows, streamk, cus):
    """m = rows + BM + 1 rows of lda = ldc = 2^20.  Stream-K: n widened until the tile count is ragged above one per CU."""
    bm, bn, k = FAR_KERNELS[kernel]
    m = rows + bm + 1
    n = bn + 1
    if streamk:
        while -(-m // bm) * -(-n // bn) <= cus or (-(-m // bm) * -(-n // bn)) % cus == 0:
            n += bn
    return m, n, k


@pytest.fixture(scope="module")
def far():
    """FAR_MAX_ROWS + 2 rows of 2^20 floats, NaN all over, allocated once for the module (9 GiB).  A and C are strided views of
    the SAME rows -- rows 1 .. m of the buffer, A in their first columns and C from column 4096 on -- so both lie past 4 GiB
    (and past 2^31 elements) without a buffer each; rows 0 and m + 1 are the rows before and after C's window."""
    import torch
    flat = torch.full(((FAR_MAX_ROWS + 2) * FAR_LD + 8,), float("nan"), device="cuda")
    yield flat
    del flat
    torch.cuda.empty_cache()


FAR_CASES = [(k, r, 0) for r in FAR_ROWS for k in FAR_KERNELS] + [(k, r, 2) for r in FAR_ROWS for k in FAR_STREAMK]


@pytest.mark.parametrize("kernel,rows,streamk", FAR_CASES, ids=[f"{k}-{r}{'-streamk' if s else ''}" for k, r, s in FAR_CASES])
def test_a_and_c_past_4_gib_stay_in_place(mm, oracle, cus, far, kernel, rows, streamk):
    """The tiles compute A + (size_t)row0 * lda and C + (size_t)row * ldc; one int product or 32-bit byte offset in a loader
    or an epilogue would send the last rows somewhere else.  The whole window against the oracle, and NaN around it: the row
    before, the row after, and 64 columns either side of every row of the window."""
    import torch
    import how_to_optimize_gemm_amd as H
    bm, bn, _ = FAR_KERNELS[kernel]
    m, n, k = far_shape(kernel, rows, streamk, cus)
    assert (m - 1) * FAR_LD * 4 >= 1 << 32 and window_ok(bm, bn, k, FAR_LD, n) and k + 64 <= FAR_C_COLUMN - 64
    a, b = oracle.harness_inputs(m, n, k, seed=m + n + k)
    c0 = np.random.default_rng(m ^ n).uniform(-1, 1, (m, n)).astype(np.float32)
    off = 1                                                 # bases 4 bytes past 16-byte alignment
    grid = _strided(far, m + 2, FAR_LD, FAR_LD, off)       # the row before, the rows of A and C, the row after
    av = grid[1:m + 1, :k]
    cv = grid[1:m + 1, FAR_C_COLUMN:FAR_C_COLUMN + n]
    around = grid[1:m + 1, FAR_C_COLUMN - 64:FAR_C_COLUMN + n + 64]
    db = torch.from_numpy(b).cuda()
    av.copy_(torch.from_numpy(a))
    try:
        with _reach(mm, kernel, streamk=streamk if streamk else (1 if kernel == "auto" else 0)):
            for accumulate in (False, True):
                if accumulate:
                    cv.copy_(torch.from_numpy(c0))
                mm.sgemm(m, n, k, av.data_ptr(), FAR_LD, db.data_ptr(), n, cv.data_ptr(), FAR_LD, accumulate,
                         torch.cuda.current_stream().cuda_stream)
                launched = H.last_launch()
                torch.cuda.synchronize()
                where = (kernel, (m, n, k), "accumulate" if accumulate else "overwrite", launched)
                if streamk:
                    assert "persistent" in launched, where
                    t, g = (int(x) for x in re.search(r"(\d+) tiles on (\d+) persistent", launched).groups())
                    assert t % g != 0 and t > cus, where
                elif kernel != "auto":
                    assert "persistent" not in launched, where
                    assert ("LDS-DMA" in launched) if "_dma" in kernel else (f"sgemm_mfma_kernel<{bm},{bn}>" in launched), where
                got = cv.cpu().numpy()
                untouched = bool(torch.isnan(grid[0]).all()) and bool(torch.isnan(grid[m + 1]).all()) and \
                    bool(torch.isnan(around[:, :64]).all()) and bool(torch.isnan(around[:, 64 + n:]).all()) and \
                    bool(torch.isnan(far[:off]).all())
                a_kept = bool(torch.equal(av.cpu(), torch.from_numpy(a)))
                around.fill_(float("nan"))
                assert untouched, (where, "wrote outside C's window")
                assert a_kept, (where, "wrote into A")
                ref = oracle.ref_mmult(a, b, c0.copy() if accumulate else None, fma=True)
                assert same_bits(got, ref), (where, first_difference(got, ref))
        assert mm.streamk_timeouts() == 0
    finally:
        grid[:m + 2, :k + 64].fill_(float("nan"))
        around.fill_(float("nan"))
