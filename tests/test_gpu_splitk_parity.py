"""The two opt-in split-K instantiations of libmmult_hip.so (sgemm_mfma_splitk_kernel, csrc/sgemm_mfma.hpp K2s, launched from
csrc/launch_reg.hip try_launch_splitk) against their own bit contract: tests/splitk_ref.py restates it from the oracle's
chains -- part s of S the ascending-k fma chain over K-slices [nk s / S, nk (s + 1) / S), part 0 started from C when
accumulating, the tile ((P0 + P1) + P2) + ... -- and every launch here must return those bits.

SPLITK_INSTANTIATIONS has one row per symbol, run with its forced id; tests/test_splitk_coverage.py holds the table to the
symbols of the built library and to the catalogue on the CPU, and tests/test_splitk_ref.py proves on the CPU that at every
shape and part count used here the restatement differs from the chain, from S - 1 and S + 1 parts and from "C added last" in
most elements: a launch that does not split, splits elsewhere or starts part 0 from zero cannot pass.

Behind the table: split-K and stream-K launches interleaved on one stream (they share the stream's hand-off words and
partial-tile slots), a split-K launch beside a stream-K launch of another stream, and split-K captured into a graph.  Every
test makes a handle of its own: the session handle is on `mfma`."""
import dataclasses
import math
import re
import types
from typing import Callable

import numpy as np
import pytest

import splitk_ref as ref
from bitcmp import first_difference, same_bits
from gpu_operands import _Options, _case, _ld, _padded, cus_fixture, handle_fixture, run_gemm
from kernel_tables import _streamk_shapes, per_cu_by_lds

pytestmark = pytest.mark.gpu

KB = 32                               # the K-slice of both tiles
FAMILY_RE = re.compile(r"^sgemm_mfma_splitk_kernel<(?P<bm>\d+),(?P<bn>\d+),(?P<wtn>\d+),(?P<wtm>\d+),(?P<kb>\d+)>$")
# symbol -> the forced id that launches it (csrc/abi.hip: Launcher::SplitK on the row's fall-back tile)
SPLITK_IDS = {"sgemm_mfma_splitk_kernel<128,128,4,4,32>": "mfma_splitk", "sgemm_mfma_splitk_kernel<128,64,2,4,32>": "mfma_splitk_128x64"}
SHARED_SHAPE = (256, 384, 224)        # the split-K shape of the shared-workspace, two-stream and graph tests: 6 tiles of 128x128


@dataclasses.dataclass(frozen=True)
class Case:
    what: str
    m: int
    n: int
    k: int
    requested: int                    # MMH_OPT_SPLITK: 0 / 1 = the "auto" count (forced id / MMH_KERNEL_AUTO), >= 2 that many parts
    auto: bool = False                # through MMH_KERNEL_AUTO (the option routes it to the 128x128 tile) instead of the forced id
    residency: bool = False           # the launcher lowers S until every part is resident: S is read from the launch string


@dataclasses.dataclass(frozen=True)
class SplitK:
    symbol: str
    kernel: str                       # the forced id
    cases: Callable                   # cus -> [Case]

    @property
    def tile(self):                   # BM, BN, KB
        g = FAMILY_RE.match(self.symbol)
        return int(g["bm"]), int(g["bn"]), int(g["kb"])


def residency_side(bm, bn, cus):
    """r of the r x r tiles that make the residency clamp bite at 8 requested parts and still leave two: 10 (100 tiles) at
    the MI355X's 256 CUs; where a device's CU count makes that idle (or too many), the smallest square count that clamps."""
    w = per_cu_by_lds(bm, bn, KB)
    if 100 * 8 > w * cus and 100 * 2 <= cus:
        return 10
    return math.isqrt(w * cus // 8) + 1


def residency_counts(bm, bn, cus, tiles, requested=8):
    """The part counts the residency clamp can leave: the largest S with tiles x S <= v x cus, for v = 1 .. w resident
    workgroups per CU (w what the LDS allows; the registers may allow fewer)."""
    return sorted({min(requested, v * cus // tiles) for v in range(1, per_cu_by_lds(bm, bn, KB) + 1)})


def _cases(bm, bn):
    def cases(cus):
        r = residency_side(bm, bn, cus)
        # 8 K-slices on the 128x128 tile (5 parts of 8 at two workgroups per CU); 16 on the 128x64 tile, whose three per CU
        # leave 7 parts: of 8 slices, 7 parts and 6 share five boundaries and half of the bits (tests/test_splitk_ref.py)
        k_res = 256 if per_cu_by_lds(bm, bn, KB) * cus // (r * r) <= 5 else 512
        out = [Case("smallest split", bm, bn, 64, 2), Case("uneven parts", bm, bn, 96, 2), Case("uneven boundaries", bm, bn, 224, 4),
               Case("first clamp", bm, bn, 96, 8), Case("several tiles", 2 * bm, 3 * bn, 224, 4)] + \
              [Case("chosen part count", bm, bn, k, 0) for k in (512, 1024, 2048)]
        if (bm, bn) == (128, 128):
            out += [Case("chosen part count, AUTO", bm, bn, k, 1, auto=True) for k in (512, 1024, 2048)]
            out += [Case("stated count, AUTO", bm, bn, 224, 4, auto=True)]
        return out + [Case("residency clamp", r * bm, r * bn, k_res, 8, residency=True)]
    return cases


def _row(symbol):
    g = FAMILY_RE.match(symbol)
    assert g, symbol
    return SplitK(symbol=symbol, kernel=SPLITK_IDS[symbol], cases=_cases(int(g["bm"]), int(g["bn"])))


SPLITK_INSTANTIATIONS = [_row(s) for s in SPLITK_IDS]


def expected_parts(case, bm, bn, cus):
    """The part count the launcher must run, restated: the option's value or policy.hip's auto count, then launch_reg.hip's
    first clamp.  (A residency case: the count BEFORE the residency clamp.)"""
    tiles = (case.m // bm) * (case.n // bn)
    S = case.requested if case.requested >= 2 else ref.auto_parts(cus, tiles, case.k)
    return ref.parts_launched(S, case.k // KB)


def inputs(m, n, k, seed=0):
    """A, B as the harness draws them and a C to accumulate onto; `seed` tells the draws of one shape apart."""
    from oracle import oracle as O
    a, b = O.harness_inputs(m, n, k, seed=(31 * m + 7 * n + k + 1000003 * seed) % (1 << 31))
    c0 = np.random.default_rng(m + n + k + seed).uniform(-1, 1, (m, n)).astype(np.float32)
    return a, b, c0


def restated(a, b, c0, S):
    """(overwrite, accumulate) of the contract; parts 1 .. S - 1 are the same chains in both and run once."""
    from oracle import oracle as O
    ps = ref.partials(O, a, b, None, S, KB)
    k1 = ref.boundaries(a.shape[1] // KB, S)[1] * KB
    first = ref.partials(O, a[:, :k1], b[:k1], c0, 1, KB)[0]
    return ref.fold(ps), ref.fold([first] + ps[1:])


def launch_words(launched):
    """(BM, BN, tiles, S) of a split-K launch string, or None."""
    g = re.search(r"sgemm_mfma_splitk_kernel<(\d+),(\d+)> .*, (\d+) tiles x (\d+) concurrent K parts", launched)
    return tuple(int(x) for x in g.groups()) if g else None


# ---- the table ------------------------------------------------------------------------------------------------------
handle = handle_fixture("mfma")
cus = cus_fixture("handle")


class _SplitK:
    """A forced kernel and MMH_OPT_SPLITK on a handle, and the defaults back afterwards."""

    def __init__(self, h, kernel, parts):
        self.h, self.kernel, self.parts = h, kernel, parts

    def __enter__(self):
        self.h.set_kernel(self.kernel)
        self.h.set_splitk(self.parts)

    def __exit__(self, *exc):
        self.h.set_splitk(0)
        self.h.set_kernel("mfma")


def _check_both_ways(h, a, b, c0, where, parts_of):
    """Overwrite and accumulate through run_gemm (NaN around C, padded leading dimensions that are multiples of 4, 16-byte
    aligned bases); parts_of(launched, where) -> the S whose restatement the bits must be."""
    want = {}
    for accumulate in (False, True):
        at = where + ("accumulate" if accumulate else "overwrite",)
        got, untouched, launched = run_gemm(h, a, b, c0 if accumulate else None, accumulate, False)
        S = parts_of(launched, at)
        if S not in want:
            want[S] = restated(a, b, c0, S)
        assert untouched, (at, "wrote outside C's window", launched)
        assert same_bits(got, want[S][accumulate]), (at, first_difference(got, want[S][accumulate]), launched)


@pytest.mark.parametrize("row", SPLITK_INSTANTIATIONS, ids=lambda r: r.symbol)
def test_every_split_k_instantiation_returns_the_restated_bits(handle, cus, row):
    bm, bn, _ = row.tile
    for case in row.cases(cus):
        tiles = (case.m // bm) * (case.n // bn)
        tile = (128, 128) if case.auto else (bm, bn)
        before = expected_parts(case, *tile, cus)

        def parts_of(launched, at):
            assert "splitk" in launched, (at, launched)
            words = launch_words(launched)
            assert words is not None and words[:3] == tile + (tiles,), (at, launched)
            if not case.residency:
                # the restated count, not the one the string reports: a launch that runs another count than it says fails the bits
                assert f"{tiles} tiles x {before} concurrent K parts" in launched, (at, before, launched)
                return before
            S = words[3]
            assert 2 <= S < before == 8 and tiles * S <= per_cu_by_lds(*tile, KB) * cus, (at, launched)
            assert S in residency_counts(*tile, cus, tiles), (at, launched)
            return S
        a, b, c0 = inputs(case.m, case.n, case.k)
        with _SplitK(handle, "auto" if case.auto else row.kernel, case.requested):
            _check_both_ways(handle, a, b, c0, (row.symbol, case), parts_of)
    assert handle.streamk_timeouts() == 0


def special_inputs(bm, bn):
    """One tile of three K-slices, three parts of one slice each.  An inf in part 0's K range (row 3), a NaN in part 1's (row
    70), a subnormal in part 2's that is all of its row (row 20: the result is subnormal), and a row of -0.0 across every part
    against positive columns of B (row 9): accumulated onto -0.0, part 0 keeps -0, parts 1 and 2 -- started from +0 -- are
    +0, and the fold is +0 where one chain would keep -0.  C holds a -inf where part 0 adds +inf to it (NaN) and one where
    it stays -inf."""
    a, b, c0 = inputs(bm, bn, 96, seed=7)
    a, b, c0 = a.copy(), b.copy(), c0.copy()
    a[3, 5] = np.inf
    b[5, 7] = 0.5
    a[70, 40] = np.nan
    a[20] = 0.0
    a[20, 70] = 1e-40
    a[9] = -0.0
    b[:, :32] = np.abs(b[:, :32]) + 0.25
    c0[9, :48] = -0.0
    c0[20, :8] = 0.0
    c0[3, 7] = -np.inf
    c0[50, 50] = -np.inf
    return a, b, c0


@pytest.mark.parametrize("row", SPLITK_INSTANTIATIONS, ids=lambda r: r.symbol)
def test_special_values_follow_the_parts(handle, oracle, row):
    bm, bn, _ = row.tile
    a, b, c0 = special_inputs(bm, bn)
    over, acc = restated(a, b, c0, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        chain = oracle.ref_mmult(a, b, c0.copy(), fma=True)
    tiny = np.finfo(np.float32).tiny
    assert np.isinf(over[3]).all() and np.isnan(over[70]).all() and np.all((over[20] != 0) & (np.abs(over[20]) < tiny))
    assert np.isnan(acc[3, 7]) and acc[50, 50] == -np.inf and np.all((acc[20, :8] != 0) & (np.abs(acc[20, :8]) < tiny))
    assert np.all(acc[9, :32] == 0) and not np.signbit(acc[9, :32]).any() and np.signbit(chain[9, :32]).all()
    assert np.all(over[9] == 0) and not np.signbit(over[9]).any()

    def parts_of(launched, at):
        assert "splitk" in launched and "1 tiles x 3 concurrent K parts" in launched, (at, launched)
        return 3
    with _SplitK(handle, row.kernel, 3):
        _check_both_ways(handle, a, b, c0, (row.symbol, "special values"), parts_of)
    assert handle.streamk_timeouts() == 0


# ---- the shared workspace --------------------------------------------------------------------------------------------
def _streamk_rows():
    """The register-staged and the K2W stream-K launch the split-K steps are interleaved with (128x128 tiles, whole shapes), as
    their rows of REG_INSTANTIATIONS and INSTANTIATIONS reach and prove them (tests/test_splitk_coverage.py holds these two to
    those rows): (row, reach)."""
    reg = types.SimpleNamespace(symbol="sgemm_mfma_streamk_kernel<128,128,false,4,4,32>", kernel="mfma", streamk=2, chain=1, persist=1,
                                markers=("sgemm_mfma_streamk_kernel<128,128>", "persistent"))
    k2w = types.SimpleNamespace(symbol="sgemm_dma5_streamk_kernel<128,128,32,4,4,3,false,true,4,2,1>", kernel="mfma_128x128_dma5", streamk=2,
                                chain=1, persist=1, markers=("sgemm_dma5_streamk_kernel<128,128>", "persistent", "chained parts"))
    return (reg, reg), (k2w, k2w)


def streamk_shapes(cus):
    """The first (ragged tile count) shape of the two stream-K rows: r x r whole tiles of five K-slices on both."""
    shape = _streamk_shapes(128, 128, False, False)(cus)[0][:3]
    return shape, shape


def test_split_k_and_stream_k_share_one_streams_workspace(handle, cus):
    """Split-K's arrival counters are the hand-off words of every stream-K family of the stream, its partial tiles lie in
    their slots, and nothing clears the words between launches: every kernel leaves them zero.  One handle, torch's
    current stream, each step's bits.  Steps 2 - 4 run the same tiles with other inputs and another S: a finisher that read
    before its producers had written would find the previous step's partials -- other numbers."""
    (reg, reg_reach), (k2w, k2w_reach) = _streamk_rows()
    reg_shape, k2w_shape = streamk_shapes(cus)
    m, n, k = SHARED_SHAPE

    def streamk(step, row, reach, shape):
        a, b, c0, want, want_acc = _case(*shape)
        with _Options(handle, reach):
            for accumulate in (False, True):
                got, untouched, launched = run_gemm(handle, a, b, c0 if accumulate else None, accumulate, False)
                at = (step, row.symbol, shape, accumulate, launched)
                for word in row.markers:
                    assert word in launched, (at, word)
                t, g = (int(x) for x in re.search(r"(\d+) tiles on (\d+) persistent", launched).groups())
                assert t % g != 0 and t > g, at               # ragged: tiles are handed over between workgroups
                assert untouched, at
                ref_ = want_acc if accumulate else want
                assert same_bits(got, ref_), (at, first_difference(got, ref_))

    def splitk(step, kernel, tile, S, seed):
        a, b, c0 = inputs(m, n, k, seed)
        tiles = (m // tile[0]) * (n // tile[1])

        def parts_of(launched, at):
            assert launch_words(launched) == tile + (tiles, S), (at, launched)
            return S
        with _SplitK(handle, kernel, S):
            _check_both_ways(handle, a, b, c0, (step, kernel, S), parts_of)

    streamk(1, reg, reg_reach, reg_shape)
    splitk(2, "mfma_splitk", (128, 128), 4, seed=1)
    splitk(3, "mfma_splitk", (128, 128), 4, seed=2)
    splitk(4, "mfma_splitk", (128, 128), 2, seed=3)
    streamk(5, k2w, k2w_reach, k2w_shape)
    splitk(6, "mfma_splitk_128x64", (128, 64), 4, seed=4)
    streamk(7, reg, reg_reach, reg_shape)
    assert handle.streamk_timeouts() == 0


# ---- two streams, and graphs ----------------------------------------------------------------------------------------------
def _operands(a, b, c_init):
    """run_gemm's operands: NaN-padded, leading dimensions that are multiples of 4, 16-byte aligned bases."""
    m, k = a.shape
    n = b.shape[1]
    _, av = _padded(m, k, _ld(k, False), 4, a)
    _, bv = _padded(k, n, _ld(n, False), 4, b)
    cflat, cv = _padded(m, n, _ld(n, False), 4, c_init)
    return av, bv, cflat, cv


def _enqueue(h, operands, m, n, k, accumulate, stream):
    """mmh_sgemm on `stream` (a torch stream) without a synchronisation; the launch string."""
    import how_to_optimize_gemm_amd as H
    av, bv, _, cv = operands
    h.sgemm(m, n, k, av.data_ptr(), _ld(k, False), bv.data_ptr(), _ld(n, False), cv.data_ptr(), _ld(n, False), accumulate, stream.cuda_stream)
    return H.last_launch()


def _window(operands, m, n):
    """(C's window, whether everything around it is still NaN)."""
    import torch
    _, _, cflat, cv = operands
    ldc = _ld(n, False)
    untouched = bool(torch.isnan(cv[:, n:]).all()) and bool(torch.isnan(cflat[:4]).all()) and bool(torch.isnan(cflat[4 + m * ldc:]).all())
    return cv[:, :n].cpu().numpy(), untouched


def test_split_k_on_a_side_stream_beside_stream_k_on_the_main_stream(cus):
    """One handle, two streams, two workspace sets (csrc/state.hip workspace_for): a split-K launch on a side stream while a
    register-staged stream-K launch runs on torch's current stream.  Neither waits for the other (the finisher's wait is for
    its own producers and bounded by the spin limit; producers never wait); both are checked after the streams are joined."""
    import torch
    import how_to_optimize_gemm_amd as H
    (reg, reach), _ = _streamk_rows()
    big, _ = streamk_shapes(cus)
    m, n, k = SHARED_SHAPE
    a1, b1, c1, want, want_acc = _case(*big)
    h = H.MMult(0, "mfma")
    try:
        side = torch.cuda.Stream()
        for accumulate in (False, True):
            a2, b2, c2 = inputs(m, n, k, seed=5 + accumulate)
            main_ops = _operands(a1, b1, c1 if accumulate else None)
            side_ops = _operands(a2, b2, c2 if accumulate else None)
            side.wait_stream(torch.cuda.current_stream())      # the fills ran on torch's current stream
            with _Options(h, reach):
                main_launch = _enqueue(h, main_ops, *big, accumulate, torch.cuda.current_stream())
            with _SplitK(h, "mfma_splitk", 4):
                side_launch = _enqueue(h, side_ops, m, n, k, accumulate, side)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            assert "persistent" in main_launch and reg.markers[0] in main_launch, main_launch
            assert launch_words(side_launch) == (128, 128, 6, 4), side_launch
            got, untouched = _window(main_ops, *big[:2])
            ref_ = want_acc if accumulate else want
            assert untouched and same_bits(got, ref_), (accumulate, main_launch, first_difference(got, ref_))
            got, untouched = _window(side_ops, m, n)
            ref_ = restated(a2, b2, c2, 4)[accumulate]
            assert untouched and same_bits(got, ref_), (accumulate, side_launch, first_difference(got, ref_))
        assert h.streamk_timeouts() == 0
    finally:
        h.close()


def test_split_k_captures_into_a_graph_on_a_stream_with_a_set_of_its_own(oracle):
    """As tests/test_gpu_round3.py::test_a_capture_never_borrows_another_streams_workspaces has it for stream-K: captured on a
    stream that owns no workspace set the call is refused (MMH_ERR_UNSUPPORTED, nothing launched); after mmh_reserve_stream
    it captures, and every replay returns the restated bits of the inputs then in the device buffers."""
    import torch
    import how_to_optimize_gemm_amd as H
    m, n, k = SHARED_SHAPE
    x1, x2 = inputs(m, n, k, seed=8), inputs(m, n, k, seed=9)
    h = H.MMult(0, "mfma_splitk")
    h.set_splitk(4)
    try:
        da, db = torch.from_numpy(x1[0]).cuda(), torch.from_numpy(x1[1]).cuda()
        c = torch.full((m, n), float("nan"), device="cuda")
        eager = h.matmul(da, db)                       # torch's current stream: code objects loaded, residency known
        assert launch_words(H.last_launch()) == (128, 128, 6, 4), H.last_launch()
        want = restated(x1[0], x1[1], x1[2], 4)
        assert same_bits(eager.cpu().numpy(), want[0]), first_difference(eager.cpu().numpy(), want[0])
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        refused = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            try:
                with torch.cuda.graph(graph, stream=side):
                    try:
                        h.matmul(da, db, out=c)
                    except H.MMultError as e:
                        refused = e
            except Exception:
                pass                                   # an empty capture may not instantiate: not what is tested
        assert refused is not None and refused.status == H.ERR_UNSUPPORTED, refused
        del refused   # (its traceback holds this frame: a dead cycle would keep `graph` until the collector runs, perhaps inside a later capture)
        torch.cuda.synchronize()
        assert bool(torch.isnan(c).all()), "a refused capture launched something"
        h.reserve_stream(side.cuda_stream, m, n, k)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                h.matmul(da, db, out=c, accumulate=True)
                captured = H.last_launch()
        assert launch_words(captured) == (128, 128, 6, 4), captured
        torch.cuda.current_stream().wait_stream(side)
        for rep, (a, b, c0) in enumerate((x1, x2, x1)):
            da.copy_(torch.from_numpy(a))
            db.copy_(torch.from_numpy(b))
            c.copy_(torch.from_numpy(c0))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            ref_ = restated(a, b, c0, 4)[1]
            assert same_bits(c.cpu().numpy(), ref_), (rep, first_difference(c.cpu().numpy(), ref_))
        assert h.streamk_timeouts() == 0
    finally:
        h.close()
