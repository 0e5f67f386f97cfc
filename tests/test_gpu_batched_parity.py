"""Every plain batched instantiation of libmmult_hip.so (csrc/sgemm_dma5.hpp sgemm_mfma_dma5_batched_kernel, launched from
csrc/launch_batched.hip) against the oracle's fused chain, bit for bit, matrix by matrix -- overwrite AND accumulate.

The kernel is one of its own: an XCD-contiguous remap of the block id, a (matrix, tile) split of the remapped id with the
launch's `first` offset, dma5_raster written out, and `accumulate`, which the fused-epilogue sibling never takes.
BATCHED_INSTANTIATIONS has one row per instantiation: three tiles x whole / guarded x four operand pairs = 24, spelled as
tests/test_batched_kernel_resources.py::_twins spells them; tests/test_batched_coverage.py holds the table to the symbols
of the built library on the CPU.  Every matrix of every case has an A, a B and a C of its own (no stride 0 in the table),
so a wrong matrix index shows in the bits.  Operand buffers hold NaN in all padding, in the gaps between matrices and in
front of the bases (tests/gpu_operands.py `Batch`), and nothing outside the C windows may change.

Behind the table: the tail split (a second launch with first != 0), launches of whole matrices where the tiles per matrix do
not divide MMH_BATCHED_MAX_WORKGROUPS (per == 3: a first grid that is no multiple of 8), special values matrix next to
matrix, and each matrix against mmh_sgemm_op on it alone."""
import dataclasses
import re

import numpy as np
import pytest

from bitcmp import first_difference, same_bits
from gpu_operands import Batch, cus_fixture, handle_fixture
from kernel_tables import FAMILY, K2W_SK, K2W_TILES, OPS, SPLIT_MARKER, TILES, _signed_zero_inputs, _special_shapes, pair_name, tail_split_case

pytestmark = pytest.mark.gpu
h = handle_fixture(check_timeouts=True, reset_kernel=True)
cus = cus_fixture("h")

TILE_HEAD = "sgemm_mfma_dma5_batched_kernel"
FAMILY_RE = re.compile(r"^sgemm_mfma_dma5_batched_kernel<(?P<bm>\d+),(?P<bn>\d+),32,\d+,\d+,3,(?P<edge>true|false),\d+,2,(?P<op>[0-3])>$")
OP_TAGS = {(0, 0): "", (1, 0): ", operands TN", (0, 1): ", operands NT", (1, 1): ", operands TT"}   # launch_dma5.hpp op_tag


def batch_tag(ops, batch):
    """What the description of a one-launch batched call ends in (before " as N launches")."""
    return OP_TAGS[tuple(ops)] + f", batch {batch}"


# ---- the table --------------------------------------------------------------------------------------------------------
def odd_stride(packed):
    """A stride past the packed matrix that is odd."""
    return packed + (1 if packed % 2 == 0 else 2)


def stored(ops, m, n, k):
    """(rows of A, columns of A, rows of B, columns of B) as the operands are stored."""
    ta, tb = ops
    return ((k, m) if ta else (m, k)) + ((n, k) if tb else (k, n))


@dataclasses.dataclass(frozen=True)
class BatchedInst:
    symbol: str
    kernel: str      # forced kernel (MMult.set_kernel)
    ops: tuple       # (transa, transb)
    guarded: bool
    bm: int
    bn: int

    def cases(self):
        """[(m, n, k, batch, extra Batch arguments)], every stride given (none is 0).  Whole: 2 x 3 tiles per matrix
        (nbm != nbn), three K-slices, ldc = n + 4, gaps of 4, 8 and 8 floats between the matrices of A, B and C, bases 16, 0
        and 32 bytes into their buffers.  Guarded: the thin edge tiles of 1 and 15, then 16 and 17, of the fused-epilogue
        table, both with a K tail; the first with packed A and B and an odd C stride, the second with every stride odd and
        bases 4, 8 and 12 bytes into their buffers."""
        if self.guarded:
            out = []
            for m, n, k, odd in ((129, 143, 77, False), (144, 145, 33, True)):
                ra, ca, rb, cb = stored(self.ops, m, n, k)
                if odd:
                    extra = {"offs": (1, 2, 3), "sa": odd_stride(ra * ca), "sb": odd_stride(rb * cb), "sc": odd_stride(m * n)}
                else:
                    extra = {"ldc": 150, "sa": ra * ca, "sb": rb * cb, "sc": m * 150 + 41}
                out.append((m, n, k, 3, extra))
            return out
        m, n, k = 2 * self.bm, 3 * self.bn, 96
        ra, ca, rb, cb = stored(self.ops, m, n, k)
        return [(m, n, k, 3, {"ldc": n + 4, "sa": ra * ca + 4, "sb": rb * cb + 8, "sc": m * (n + 4) + 8, "offs": (4, 0, 8)})]


def _table_rows():
    for t in K2W_SK:
        bm, bn = (int(x) for x in t.split(",")[:2])
        for edge in ("false", "true"):
            for op in range(4):
                yield BatchedInst(symbol=f"{TILE_HEAD}<{t},{edge},{K2W_TILES[t]},{op}>", kernel=f"mfma_{bm}x{bn}_dma5",
                                  ops=(op & 1, op >> 1), guarded=edge == "true", bm=bm, bn=bn)


BATCHED_INSTANTIATIONS = list(_table_rows())


class Expected(Batch):
    """A Batch that keeps every matrix's oracle results (the rows and tests that share a batch share them)."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self._want = {}

    def want(self, oracle, i, accumulate):
        key = (i, bool(accumulate))
        if key not in self._want:
            with np.errstate(over="ignore", invalid="ignore", under="ignore"):
                self._want[key] = super().want(oracle, i, accumulate)
        return self._want[key]

    def run_launch(self, h, accumulate):
        """(C's whole buffer afterwards, the launch text)."""
        import how_to_optimize_gemm_amd as H
        got = self.run(h, accumulate=accumulate)
        return got, H.last_launch()

    def check_bits(self, oracle, got, accumulate, where):
        inside = np.zeros(got.shape, dtype=bool)
        for i in range(self.batch):
            want, win = self.want(oracle, i, accumulate), self.c_window(got, i)
            assert same_bits(win, want), (where, "matrix", i, first_difference(win, want))
            o = self.offs[2] + i * self.sc
            inside[o:o + self.m * self.ldc].reshape(self.m, self.ldc)[:, :self.n] = True
        assert same_bits(got[~inside], self.c0[~inside]), (where, "wrote outside the C matrices")

    def alone(self, h, i, accumulate):
        """Matrix i through mmh_sgemm_op, on dense buffers of its own."""
        import torch
        a, b = self.logical(i)
        sa = torch.from_numpy(np.ascontiguousarray(a.T if self.ta else a)).cuda()
        sb = torch.from_numpy(np.ascontiguousarray(b.T if self.tb else b)).cuda()
        c = torch.from_numpy(self.cm[i]).cuda() if accumulate else torch.full((self.m, self.n), float("nan"), device="cuda")
        h.sgemm_op(self.ta, self.tb, self.m, self.n, self.k, sa.data_ptr(), self.m if self.ta else self.k, sb.data_ptr(),
                   self.k if self.tb else self.n, c.data_ptr(), self.n, accumulate, torch.cuda.current_stream().cuda_stream)
        return c.cpu().numpy()


def _row_batches(inst):
    for m, n, k, batch, extra in inst.cases():
        bt = Expected(*inst.ops, m, n, k, batch, seed=m + 3 * n + 5 * k + 7 * inst.ops[0] + 11 * inst.ops[1], **extra)
        assert bt.sa and bt.sb and bt.sc, "every matrix has operands of its own"
        yield (m, n, k), bt


@pytest.mark.parametrize("inst", BATCHED_INSTANTIATIONS, ids=lambda i: i.symbol)
def test_every_batched_instantiation_returns_the_oracle_bits(h, oracle, inst):
    h.set_kernel(inst.kernel)
    try:
        for shape, bt in _row_batches(inst):
            for accumulate in (False, True):
                where = (inst.symbol, shape, "accumulate" if accumulate else "overwrite")
                got, launched = bt.run_launch(h, accumulate)
                print(where, launched)
                assert launched.startswith(f"{TILE_HEAD}<{inst.bm},{inst.bn}>"), (where, launched)
                assert ("guarded" in launched) == inst.guarded, (where, launched)
                assert launched.endswith(batch_tag(inst.ops, bt.batch)), (where, launched)
                bt.check_bits(oracle, got, accumulate, where)
    finally:
        h.set_kernel("auto")


@pytest.mark.parametrize("inst", BATCHED_INSTANTIATIONS, ids=lambda i: i.symbol)
def test_each_matrix_alone_gives_the_batched_calls_bits(h, inst):
    """The first, the middle and the last matrix of every case of every row: mmh_sgemm_op on that matrix alone, overwrite and
    accumulate, gives the bits the batched call left in its window."""
    h.set_kernel(inst.kernel)
    try:
        for shape, bt in _row_batches(inst):
            for accumulate in (False, True):
                got, launched = bt.run_launch(h, accumulate)
                assert launched.startswith(f"{TILE_HEAD}<{inst.bm},{inst.bn}>"), launched
                for i in sorted({0, bt.batch // 2, bt.batch - 1}):
                    one = bt.alone(h, i, accumulate)
                    assert same_bits(one, bt.c_window(got, i)), (inst.symbol, shape, accumulate, "differs from mmh_sgemm_op on matrix", i,
                                                                  first_difference(bt.c_window(got, i), one))
    finally:
        h.set_kernel("auto")


# ---- the tail split ---------------------------------------------------------------------------------------------------
# (sa, sb, accumulate): overwrite with an A per matrix and one B; accumulate with one A and one B -- the C matrices, which the
# chains start from, tell the matrices, and with them the ids of the second launch, apart
SPLIT_RUNS = {"overwrite, an A per matrix": (None, 0, False), "accumulate, a C per matrix": (0, 0, True)}


@pytest.mark.parametrize("name", list(SPLIT_RUNS))
def test_a_batch_whose_last_round_is_one_tile_per_cu_goes_out_split(h, oracle, cus, name):
    """CUs matrices of 2 x 2 tiles on the 64x64 tile (three workgroups per CU): three whole rounds as one launch, the fourth --
    the last quarter of the batch -- as a launch of its own whose ids start at first = 3 CUs."""
    sa, sb, accumulate = SPLIT_RUNS[name]
    m, n, k, batch = tail_split_case(cus)
    bt = Expected(0, 1, m, n, k, batch, seed=6, sa=sa, sb=sb)
    h.set_kernel("mfma_64x64_dma5")
    try:
        got, launched = bt.run_launch(h, accumulate)
        print(name, launched)
        assert launched.startswith(TILE_HEAD + "<64,64>") and SPLIT_MARKER in launched and "guarded" not in launched, launched
        assert launched.endswith(batch_tag((0, 1), batch) + " as 2 launches"), launched
        bt.check_bits(oracle, got, accumulate, ("tail split", name))
    finally:
        h.set_kernel("auto")


# ---- launches of whole matrices, three tiles each -----------------------------------------------------------------------
PER3 = dict(m=129, n=1, k=1, lda=1, ldb=1, ldc=1, sa=0, sb=1, sc=129)   # 129 rows: two 64-row tiles and a thin one of 1


def per3_batch(max_workgroups):
    """Two matrices more than one launch of whole matrices holds at three tiles a matrix."""
    return max_workgroups // 3 + 2


def test_launches_of_whole_matrices_at_three_tiles_a_matrix(h):
    """C_i = a b_i: one column A that every matrix shares, a B of one element per matrix, C_i 129 x 1 -- packed, 0.72 GB.  The cap
    is no multiple of 3: the first launch holds cap // 3 whole matrices (4194303 workgroups, no multiple of 8: the XCD runs
    are of two lengths), the second the last two.  One rounding of one product onto +0 per element."""
    import torch
    import how_to_optimize_gemm_amd as H
    p = PER3
    batch = per3_batch(H.BATCHED_MAX_WORKGROUPS)
    g = torch.Generator(device="cuda").manual_seed(8)
    a = torch.rand(p["m"], device="cuda", generator=g) + 0.5
    b = torch.rand(batch, device="cuda", generator=g) + 0.5
    c = torch.full((batch * p["sc"],), float("nan"), device="cuda")
    h.set_kernel("mfma_64x64_dma5")
    try:
        h.sgemm_batched(0, 0, p["m"], p["n"], p["k"], a.data_ptr(), p["lda"], p["sa"], b.data_ptr(), p["ldb"], p["sb"], c.data_ptr(),
                        p["ldc"], p["sc"], batch, False, torch.cuda.current_stream().cuda_stream)
        launched = H.last_launch()
        torch.cuda.synchronize()
    finally:
        h.set_kernel("auto")
    print(launched)
    assert launched.startswith(TILE_HEAD + "<64,64>") and "guarded" in launched, launched
    assert launched.endswith(f", batch {batch} as 2 launches"), launched
    an, bn = a.cpu().numpy(), b.cpu().numpy()
    assert an.min() >= 0.5 and an.max() <= 1.5 and bn.min() >= 0.5 and bn.max() <= 1.5
    want = (bn[:, None] * an[None, :]).astype(np.float32)          # want[i, r] = C_i[r] = a[r] b[i]
    got = c.cpu().numpy().reshape(batch, p["sc"])
    del c
    torch.cuda.empty_cache()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


# ---- special values, matrix next to matrix ------------------------------------------------------------------------------
SPECIAL_NAMES = ("overflow", "subnormal", "inf/nan", "signed zero")   # the NaN matrix between two that hold no NaN
SPECIAL_CASES = [(kernel, ops) for kernel in TILES for ops in OPS.values()]


def special_batch(oracle, ops, m, n, k, guarded):
    """One batch of four matrices: the overflow, subnormal, inf / NaN and signed-zero blocks of
    tests/test_gpu_lds_dma_parity.py::test_special_values_follow_the_chain_on_the_lds_dma_tiles, each with its own A, B and C
    (the signed-zero block's C is -0 where every product is -0).  Returns (the batch, the signed-zero mask)."""
    a, b = oracle.harness_inputs(m, n, k, seed=99 + k)
    a_p, b_p = a.copy(), b.copy()
    a_p[3, 5], a_p[70, 10], b_p[5, 7], b_p[20, 100] = np.inf, -np.inf, 0.0, np.nan
    a_z, b_z, c_z, neg_zero = _signed_zero_inputs(a, b)
    As = [(a * np.float32(3e19)).astype(np.float32), (a * np.float32(1e-21)).astype(np.float32), a_p, a_z]
    Bs = [(b * np.float32(3e19)).astype(np.float32), (b * np.float32(1e-21)).astype(np.float32), b_p, b_z]
    rng = np.random.default_rng(17)
    c_r = [rng.uniform(-1, 1, (m, n)).astype(np.float32) for _ in range(3)]
    Cs = [c_r[0], (c_r[1] * np.float32(1e-41)).astype(np.float32), c_r[2], c_z]   # (accumulate: the subnormal sums start subnormal)
    fill = lambda mats, t: (lambda r, c, it=iter(mats): np.ascontiguousarray(next(it).T if t else next(it)))
    ldc = n + (1 if n % 2 == 0 else 2) if guarded else n + 4
    ra, ca, rb, cb = stored(ops, m, n, k)
    gaps, offs = ((1, 3, 5), (1, 2, 3)) if guarded else ((4, 8, 8), (4, 0, 8))
    sa, sb, sc = ra * ca + gaps[0], rb * cb + gaps[1], m * ldc + gaps[2]
    bt = Expected(*ops, m, n, k, 4, seed=1, ldc=ldc, sa=sa, sb=sb, sc=sc, offs=offs, a_val=fill(As, ops[0]), b_val=fill(Bs, ops[1]),
                  c_val=fill(Cs, 0))
    return bt, neg_zero


def check_special_expectation(want, neg_zero, accumulate):
    """What each block is there for really occurs in the oracle's results (want: the four matrices'), and the NaN matrix's
    neighbours hold no NaN: one found there came from the wrong matrix."""
    over, sub, planted, zero = want
    assert np.isinf(over).any()
    assert np.any((sub != 0) & (np.abs(sub) < np.finfo(np.float32).tiny)), "must reach subnormals"
    assert np.isnan(planted[3, 7]) and np.isnan(planted[:, 100]).all() and np.isinf(planted[70]).any()
    assert np.isfinite(planted).any() and not np.isnan(sub).any() and not np.isnan(zero).any()
    z = zero[neg_zero]
    assert (z == 0).all() and (np.signbit(z).all() if accumulate else not np.signbit(z).any())


@pytest.mark.parametrize("kernel,ops", SPECIAL_CASES, ids=[f"{k}_{pair_name(o)}" for k, o in SPECIAL_CASES])
def test_special_values_stay_in_their_own_matrix(h, oracle, kernel, ops):
    """Subnormals, overflow to inf, planted inf / NaN and signed zeros (overwrite: +0, accumulate onto -0: -0) as the four
    matrices of ONE batch, on the tile's whole shape and on its guarded one with a K tail, overwrite and accumulate.  The
    NaN matrix lies between two that hold no NaN."""
    failures = []
    h.set_kernel(kernel)
    try:
        for m, n, k, guarded in _special_shapes(kernel):
            bt, neg_zero = special_batch(oracle, ops, m, n, k, guarded)
            for accumulate in (False, True):
                want = [bt.want(oracle, i, accumulate) for i in range(4)]
                check_special_expectation(want, neg_zero, accumulate)
                got, launched = bt.run_launch(h, accumulate)
                where = (kernel, pair_name(ops), (m, n, k), "accumulate" if accumulate else "overwrite")
                assert launched.startswith(TILE_HEAD + FAMILY[kernel]) and ("guarded" in launched) == guarded, (where, launched)
                assert launched.endswith(batch_tag(ops, 4)), (where, launched)
                inside = np.zeros(got.shape, dtype=bool)
                for i in range(4):
                    win = bt.c_window(got, i)
                    if not same_bits(win, want[i]):
                        failures.append(f"{where} {SPECIAL_NAMES[i]}: {first_difference(win, want[i])}  [{launched}]")
                    o = bt.offs[2] + i * bt.sc
                    inside[o:o + m * bt.ldc].reshape(m, bt.ldc)[:, :n] = True
                assert same_bits(got[~inside], bt.c0[~inside]), (where, "wrote outside the C matrices")
    finally:
        h.set_kernel("auto")
    assert not failures, "\n".join(failures)
