"""Strided batched SGEMM with the fused epilogue on the GPU (mmh_sgemm_batched_ex, MMult.baddbmm, MMult.batched_linear;
csrc/launch_batched_ex.hip, csrc/sgemm_dma5.hpp sgemm_mfma_dma5_batched_ex_kernel):
C_i = act(alpha op(A_i) op(B_i) + beta C_i + bias_i) for every matrix of a batch, matrix i at base + i * stride, its bias at
dBias + i * strideBias.  The contract is mmh_sgemm_ex's, matrix by matrix.

The expectation is built HERE from the pinned oracle's fused chain and float32 numpy, one operation at a time
(tests/ex_ref.py `expected`), never from the library; results are compared as 32-bit patterns.  Operand buffers hold NaN
in all padding, in the gaps between matrices and in front of the bases (tests/gpu_operands.py `Batch`), and nothing
outside the C windows may change.

BATCHED_EX_INSTANTIATIONS has one row per instantiation: three tiles x whole / guarded x four operand pairs = 24;
tests/test_batched_ex_coverage.py holds the table to the symbols of the built library on the CPU."""
import dataclasses
import functools
import re

import numpy as np
import pytest

from bitcmp import first_difference, same_bits
from ex_ref import COL, NONE, RELU, ROW, expected
from gpu_operands import Batch, cus_fixture, handle_fixture
from kernel_tables import (FAMILY, K2W_SK, K2W_TILES, OPS, SPLIT_MARKER, TILES, _special_shapes, ex_tag, pair_name, special_blocks,
                           tail_split, tail_split_case)   # noqa: F401 (tail_split: tests/test_batched_ex_coverage.py reads it here)

pytestmark = pytest.mark.gpu
h = handle_fixture(check_timeouts=True)
cus = cus_fixture("h")

KERNELS = ["auto"] + TILES + ["naive"]
TILE_HEAD = "sgemm_mfma_dma5_batched_ex_kernel"
NAIVE_HEAD = "sgemm_naive_batched_ex_kernel"
# name: alpha, beta, bias mode, activation.  beta == 0 runs over C buffers that are NaN throughout: C must not be read.
EPILOGUES = {"identity": (1.0, 0.0, NONE, 0), "all": (-1.3, 0.5, COL, RELU), "row_bias": (1.0, 0.0, ROW, 0)}
# The smallest cube on the 128 grid, from 2176 upwards, whose batch of 2 (NT) mmh_auto_plan_batched_ex plans as a loop of the
# per-matrix `ex` plan on 256 CUs (tests/test_batched_ex_coverage.py holds the number to the planner).
LOOP_CUBE = 2176


def per_matrix_stride(length):
    """A bias stride >= length that is no multiple of 4."""
    return length + (1 if (length + 1) % 4 else 2)


class ExBatch(Batch):
    """Batch with a column and a row bias per matrix: bias_i at bias_off + i * stride in a NaN buffer (stride 0: one bias for the
    whole batch).  sbias: {COL: stride, ROW: stride}; the default is per matrix, no multiple of 4."""

    def __init__(self, ta, tb, m, n, k, batch, seed, sbias=None, bias_off=1, bias_val=None, **kw):
        super().__init__(ta, tb, m, n, k, batch, seed, **kw)
        rng = np.random.default_rng(seed + 1000)
        self.bias_off = bias_off
        self.sbias = {COL: per_matrix_stride(n), ROW: per_matrix_stride(m), **(sbias or {})}
        self.bias_flat, self.bias_vecs = {}, {}
        for mode, length in ((COL, n), (ROW, m)):
            s = self.sbias[mode]
            count = batch if s else 1
            flat = np.full(bias_off + (count - 1) * s + length + 5, np.nan, np.float32)
            vecs = []
            for i in range(count):
                v = bias_val[mode] if bias_val and bias_val.get(mode) is not None else rng.uniform(-1, 1, length).astype(np.float32)
                flat[bias_off + i * s:bias_off + i * s + length] = v
                vecs.append(v)
            self.bias_flat[mode], self.bias_vecs[mode] = flat, vecs
        self._chain = {}

    def bias(self, mode, i):
        return None if mode == NONE else self.bias_vecs[mode][i if self.sbias[mode] else 0]

    def chain(self, oracle, i):
        key = (i if self.sa else 0, i if self.sb else 0)
        if key not in self._chain:
            a, b = self.logical(i)
            with np.errstate(over="ignore", invalid="ignore"):
                self._chain[key] = oracle.ref_mmult(a, b, fma=True)
        return self._chain[key]

    def want_ex(self, oracle, i, alpha, beta, mode, act):
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            return expected(self.chain(oracle, i), alpha, beta, self.cm[i], self.bias(mode, i), mode, act)

    def c_before(self, beta):
        return self.c0 if beta != 0 else np.full_like(self.c0, np.nan)

    def run_ex(self, h, alpha, beta, mode, act, stream=None):
        """The call on fresh device buffers; (C's whole buffer afterwards, the launch text)."""
        import torch
        import how_to_optimize_gemm_amd as H
        da, db, dc = (torch.from_numpy(x).cuda() for x in (self.a, self.b, self.c_before(beta)))
        pbias = 0
        if mode != NONE:
            dbias = torch.from_numpy(self.bias_flat[mode]).cuda()
            pbias = dbias.data_ptr() + 4 * self.bias_off
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        h.sgemm_batched_ex(self.ta, self.tb, self.m, self.n, self.k, alpha, da.data_ptr() + 4 * self.offs[0], self.lda, self.sa,
                           db.data_ptr() + 4 * self.offs[1], self.ldb, self.sb, beta, dc.data_ptr() + 4 * self.offs[2], self.ldc,
                           self.sc, self.batch, pbias, self.sbias[mode] if mode != NONE else 0, mode, act, s)
        launched = H.last_launch()
        torch.cuda.synchronize()
        return dc.cpu().numpy(), launched

    def check_ex(self, oracle, got, epilogue, where):
        alpha, beta, mode, act = epilogue
        inside = np.zeros(got.shape, dtype=bool)
        for i in range(self.batch):
            want = self.want_ex(oracle, i, alpha, beta, mode, act)
            win = self.c_window(got, i)
            assert same_bits(win, want), (where, "matrix", i, first_difference(win, want))
            o = self.offs[2] + i * self.sc
            inside[o:o + self.m * self.ldc].reshape(self.m, self.ldc)[:, :self.n] = True
        assert same_bits(got[~inside], self.c_before(beta)[~inside]), (where, "wrote outside the C matrices")

    def alone(self, h, i, epilogue):
        """Matrix i through mmh_sgemm_ex, on dense buffers of its own."""
        import torch
        alpha, beta, mode, act = epilogue
        a, b = self.logical(i)
        sa = torch.from_numpy(np.ascontiguousarray(a.T if self.ta else a)).cuda()
        sb = torch.from_numpy(np.ascontiguousarray(b.T if self.tb else b)).cuda()
        c = torch.from_numpy(self.cm[i] if beta != 0 else np.full((self.m, self.n), np.nan, np.float32)).cuda()
        bias = None if mode == NONE else torch.from_numpy(self.bias(mode, i)).cuda()
        h.sgemm_ex(self.ta, self.tb, self.m, self.n, self.k, alpha, sa.data_ptr(), self.m if self.ta else self.k, sb.data_ptr(),
                   self.k if self.tb else self.n, beta, c.data_ptr(), self.n, bias.data_ptr() if bias is not None else 0, mode, act,
                   torch.cuda.current_stream().cuda_stream)
        return c.cpu().numpy()

    def check_alone(self, h, got, epilogue, where):
        """Matrices 0, batch / 2 and batch - 1: mmh_sgemm_ex on that matrix alone gives the batched call's bits."""
        for i in sorted({0, self.batch // 2, self.batch - 1}):
            assert same_bits(self.alone(h, i, epilogue), self.c_window(got, i)), (where, "differs from mmh_sgemm_ex on matrix", i)


def batch_tag(ops, epilogue, batch):
    """What the description of a one-launch or naive batched `ex` call ends in."""
    return ex_tag(ops, *epilogue) + f", batch {batch}"


# ---- the table --------------------------------------------------------------------------------------------------------
FAMILY_RE = re.compile(r"^sgemm_mfma_dma5_batched_ex_kernel<(?P<bm>\d+),(?P<bn>\d+),32,\d+,\d+,3,(?P<edge>true|false),\d+,2,(?P<op>[0-3])>$")


@dataclasses.dataclass(frozen=True)
class BatchedExInst:
    symbol: str
    kernel: str      # forced kernel (MMult.set_kernel)
    ops: tuple       # (transa, transb)
    guarded: bool
    bm: int
    bn: int

    def cases(self):
        """[(m, n, k, batch, extra Batch arguments)].  Whole: more than one tile per matrix, every leading dimension, stride and
        base a multiple of 4 floats, gaps between the matrices.  Guarded: thin edge tiles of 1 and 15, then 16 and 17, with a
        K tail, and strides / bases that are no multiples of 4 (the shapes of tests/test_gpu_batched.py)."""
        if self.guarded:
            return [(129, 143, 77, 3, {"ldc": 150, "sc": 129 * 150 + 41}), (144, 145, 33, 3, {"offs": (1, 2, 3)})]
        m, n = 2 * self.bm, self.bn
        return [(m, n, 64, 3, {"ldc": n + 4, "sc": m * (n + 4) + 8, "offs": (4, 0, 8)})]


def _table_rows():
    for t in K2W_SK:
        bm, bn = (int(x) for x in t.split(",")[:2])
        for edge in ("false", "true"):
            for op in range(4):
                yield BatchedExInst(symbol=f"{TILE_HEAD}<{t},{edge},{K2W_TILES[t]},{op}>", kernel=f"mfma_{bm}x{bn}_dma5",
                                    ops=(op & 1, op >> 1), guarded=edge == "true", bm=bm, bn=bn)


BATCHED_EX_INSTANTIATIONS = list(_table_rows())


@functools.lru_cache(maxsize=8)
def _table_batch(ops, m, n, k, batch, extra):
    return ExBatch(*ops, m, n, k, batch, seed=m + 3 * n + 5 * k + 7 * ops[0] + 11 * ops[1], **dict(extra))


@pytest.mark.parametrize("inst", BATCHED_EX_INSTANTIATIONS, ids=lambda i: i.symbol)
def test_every_batched_ex_instantiation_returns_the_contract_bits(h, oracle, inst):
    h.set_kernel(inst.kernel)
    try:
        for m, n, k, batch, extra in inst.cases():
            bt = _table_batch(inst.ops, m, n, k, batch, tuple(sorted(extra.items())))
            assert bt.sbias[COL] % 4 and bt.sbias[ROW] % 4
            for name, ep in EPILOGUES.items():
                where = (inst.symbol, (m, n, k), name)
                got, launched = bt.run_ex(h, *ep)
                print(where, launched)
                assert launched.startswith(f"{TILE_HEAD}<{inst.bm},{inst.bn}>"), (where, launched)
                assert ("guarded" in launched) == inst.guarded, (where, launched)
                assert launched.endswith(batch_tag(inst.ops, ep, batch)), (where, launched)
                bt.check_ex(oracle, got, ep, where)
                bt.check_alone(h, got, ep, where)
    finally:
        h.set_kernel("auto")


# ---- strides, broadcasts, shared biases ---------------------------------------------------------------------------------
# name: (m, n, k, batch, extra ExBatch arguments, must be guarded on a tile)
CASES = {
    "strides_not_mult_of_4": (64, 96, 64, 5, {"sa": 64 * 64 + 1, "sb": 64 * 96 + 3, "sc": 64 * 96 + 5}, True),
    "broadcast_a": (100, 72, 40, 6, {"sa": 0, "sc": 100 * 72 + 8}, False),
    "broadcast_b": (72, 100, 40, 6, {"sb": 0, "sc": 72 * 100 + 8}, False),
    "shared_biases": (72, 100, 40, 4, {"sbias": {COL: 0, ROW: 0}, "sc": 72 * 100 + 8}, False),
}


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("name", list(CASES))
def test_strides_broadcasts_and_shared_biases(h, oracle, name, op):
    m, n, k, batch, extra, guarded = CASES[name]
    bt = ExBatch(*OPS[op], m, n, k, batch, seed=sum(map(ord, name)) + 3, **extra)
    try:
        for kern in KERNELS:
            h.set_kernel(kern)
            for ename, ep in EPILOGUES.items():
                where = (kern, op, name, ename)
                got, launched = bt.run_ex(h, *ep)
                bt.check_ex(oracle, got, ep, where)
                assert launched.endswith(batch_tag(OPS[op], ep, batch)), (where, launched)   # (AUTO: none of these folds)
                if kern == "naive":
                    assert launched.startswith(NAIVE_HEAD), launched
                else:
                    assert launched.startswith(TILE_HEAD + FAMILY.get(kern, "<")), (where, launched)
                    if guarded:
                        assert "guarded" in launched, (where, launched)
                if kern == "auto":
                    bt.check_alone(h, got, ep, where)
    finally:
        h.set_kernel("auto")


@pytest.mark.parametrize("op", ["NN", "NT"])
def test_many_small_matrices_cross_the_xcd_runs(h, oracle, op):
    """512 x 64^3: one tile per matrix, so the remapped block id IS the matrix -- every matrix has operands and biases of its own."""
    bt = ExBatch(*OPS[op], 64, 64, 64, 512, seed=77)
    try:
        for kern in ("auto", "mfma_64x64_dma5"):
            h.set_kernel(kern)
            for ename in ("all", "row_bias"):
                got, launched = bt.run_ex(h, *EPILOGUES[ename])
                assert launched.startswith(TILE_HEAD) and launched.endswith(batch_tag(OPS[op], EPILOGUES[ename], 512)), launched
                bt.check_ex(oracle, got, EPILOGUES[ename], (kern, op, ename))
    finally:
        h.set_kernel("auto")


# ---- the tail split ---------------------------------------------------------------------------------------------------
def test_a_batch_whose_last_round_is_one_tile_per_cu_goes_out_split(h, oracle, cus):
    """A and B are shared (stride 0): one oracle chain serves every matrix, and the per-matrix biases and C matrices tell the
    matrices -- and with them the ids of the second launch -- apart."""
    m, n, k, batch = tail_split_case(cus)
    bt = ExBatch(0, 1, m, n, k, batch, seed=5, sa=0, sb=0)
    h.set_kernel("mfma_64x64_dma5")
    try:
        for ename in ("all", "row_bias"):
            got, launched = bt.run_ex(h, *EPILOGUES[ename])
            assert launched.startswith(TILE_HEAD + "<64,64>") and SPLIT_MARKER in launched, launched
            assert launched.endswith(batch_tag((0, 1), EPILOGUES[ename], batch) + " as 2 launches"), launched
            bt.check_ex(oracle, got, EPILOGUES[ename], ("tail split", ename))
    finally:
        h.set_kernel("auto")


# ---- the workgroup cap ------------------------------------------------------------------------------------------------
def test_a_batch_beyond_the_workgroup_cap_advances_the_per_matrix_biases(h):
    """tests/test_gpu_batched.py's cap test with an epilogue: 1x1x1 matrices, one float of bias each (stride_bias = 1), ReLU.  A
    launch of a later chunk that did not advance its bias pointer would give the matrices behind the cap the first ones' biases.
    The expectation is float32 numpy, one rounding per operation: r = fl(fl(a b) + bias), r where r > 0, else +0."""
    import torch
    import how_to_optimize_gemm_amd as H
    batch = H.BATCHED_MAX_WORKGROUPS + 4097
    g = torch.Generator(device="cuda").manual_seed(6)
    a, b, bias = (torch.rand(batch, device="cuda", generator=g) * 2 - 1 for _ in range(3))
    r = a.cpu().numpy() * b.cpu().numpy() + bias.cpu().numpy()
    assert r.dtype == np.float32
    want = np.where(r > 0, r, np.float32(0.0)).astype(np.float32)
    naive_launches = -(-batch // 65535)
    try:
        for kern, head, tail in (("auto", TILE_HEAD, "as 2 launches"), ("naive", NAIVE_HEAD, f"as {naive_launches} launches")):
            h.set_kernel(kern)
            c = torch.full((batch,), float("nan"), device="cuda")
            h.sgemm_batched_ex(0, 0, 1, 1, 1, 1.0, a.data_ptr(), 1, 1, b.data_ptr(), 1, 1, 0.0, c.data_ptr(), 1, 1, batch,
                               bias.data_ptr(), 1, COL, RELU, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            launch = H.last_launch()
            assert head in launch and launch.endswith(f", batch {batch} {tail}"), (kern, launch)
            got = c.cpu().numpy()
            assert same_bits(got, want), (kern, first_difference(got.reshape(1, -1), want.reshape(1, -1)))
    finally:
        h.set_kernel("auto")


# ---- AUTO's forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["NN", "NT"])
def test_auto_folds_a_shared_b_with_foldable_biases(h, oracle, op):
    m, n, k, batch = 128, 128, 64, 8
    fold = f", batch {batch} folded into one {batch * m}-row GEMM"
    h.set_kernel("auto")
    # no bias; a column bias the batch shares; row biases packed m apart: all fold
    bt = ExBatch(*OPS[op], m, n, k, batch, seed=21, sb=0, sbias={COL: 0, ROW: m})
    for ep in ((0.7, 0.5, NONE, 0), EPILOGUES["all"], (1.0, 0.0, ROW, RELU)):
        got, launched = bt.run_ex(h, *ep)
        assert launched.endswith(ex_tag(OPS[op], *ep) + fold), launched
        bt.check_ex(oracle, got, ep, (op, ep))
        bt.check_alone(h, got, ep, (op, ep))
    # a column bias per matrix, a shared row bias: one launch
    bt = ExBatch(*OPS[op], m, n, k, batch, seed=22, sb=0, sbias={COL: n, ROW: 0})
    for ep in (EPILOGUES["all"], EPILOGUES["row_bias"]):
        got, launched = bt.run_ex(h, *ep)
        assert launched.startswith(TILE_HEAD) and launched.endswith(batch_tag(OPS[op], ep, batch)), launched
        bt.check_ex(oracle, got, ep, (op, ep))


def test_auto_loops_over_two_large_matrices(h, oracle):
    N = LOOP_CUBE
    ep = EPILOGUES["all"]
    bt = ExBatch(0, 1, N, N, N, 2, seed=31)
    try:
        for kern in ["auto"] + TILES:
            h.set_kernel(kern)
            got, launched = bt.run_ex(h, *ep)
            if kern == "auto":
                assert launched.endswith(ex_tag((0, 1), *ep) + ", batch 2 as a loop of 2 per-matrix launches"), launched
            else:
                assert launched.startswith(TILE_HEAD + FAMILY[kern]) and launched.endswith(batch_tag((0, 1), ep, 2)), launched
            bt.check_ex(oracle, got, ep, (kern, N))
    finally:
        h.set_kernel("auto")


# ---- special values ---------------------------------------------------------------------------------------------------
SPECIAL_CASES = [(kernel, ops) for kernel in ["naive"] + TILES for ops in OPS.values()]


@pytest.mark.parametrize("kernel,ops", SPECIAL_CASES, ids=[f"{k}_{pair_name(o)}" for k, o in SPECIAL_CASES])
def test_special_values_follow_the_epilogue_contract(h, oracle, kernel, ops):
    """The blocks of tests/test_gpu_ex_parity.py (+-inf, -0 chains through ReLU, NaN through ReLU, alpha == 0 with inf products,
    NaN in C with beta != 0, overflow inside the epilogue, subnormal beta c) in every matrix of a batch of 3, on one whole and
    one guarded shape per tile and on the naive kernel.  The matrices share the block's operands, C and bias values at
    addresses of their own."""
    failures = []
    h.set_kernel(kernel)
    try:
        for m, n, k, guarded in _special_shapes(kernel):
            for blk in special_blocks(oracle, m, n, k):
                blk.check_expectation()
                sa = np.ascontiguousarray(blk.a.T if ops[0] else blk.a)
                sb = np.ascontiguousarray(blk.b.T if ops[1] else blk.b)
                extra = {"offs": (1, 2, 3), "ldc": n + (1 if n % 2 == 0 else 2)} if guarded else {"offs": (4, 0, 8), "ldc": n + 4}
                c_val = (lambda r, c, x=blk.c: x.copy()) if blk.c is not None else None
                bt = ExBatch(*ops, m, n, k, 3, seed=1, a_val=lambda r, c: sa, b_val=lambda r, c: sb, c_val=c_val,
                             sc=m * extra["ldc"] + (5 if guarded else 8), bias_val={blk.mode: blk.bias}, **extra)
                ep = (blk.alpha, blk.beta, blk.mode, blk.act)
                got, launched = bt.run_ex(h, *ep)
                where = (kernel, pair_name(ops), (m, n, k), blk.name)
                assert launched.endswith(batch_tag(ops, ep, 3)), (where, launched)
                if kernel == "naive":
                    assert launched.startswith(NAIVE_HEAD), launched
                else:
                    assert launched.startswith(TILE_HEAD + FAMILY[kernel]) and ("guarded" in launched) == guarded, (where, launched)
                c_before = bt.c_before(blk.beta)
                inside = np.zeros(got.shape, dtype=bool)
                for i in range(3):
                    win = bt.c_window(got, i)
                    if not same_bits(win, blk.want):
                        failures.append(f"{where} matrix {i}: {first_difference(win, blk.want)}  [{launched}]")
                    o = bt.offs[2] + i * bt.sc
                    inside[o:o + m * bt.ldc].reshape(m, bt.ldc)[:, :n] = True
                assert same_bits(got[~inside], c_before[~inside]), (where, "wrote outside the C matrices")
    finally:
        h.set_kernel("auto")
    assert not failures, "\n".join(failures)


# ---- empty cases and refusals -------------------------------------------------------------------------------------------
def test_empty_cases_and_refusals_leave_c_untouched(h):
    import torch
    import how_to_optimize_gemm_amd as H
    s = torch.cuda.current_stream().cuda_stream
    m, n, k, batch = 40, 50, 30, 4
    ldc, sc = 52, 40 * 52 + 7
    g = torch.Generator(device="cuda").manual_seed(1)
    a = torch.rand(batch * m * k, device="cuda", generator=g)
    b = torch.rand(batch * k * n, device="cuda", generator=g)
    bias = torch.rand(batch * n, device="cuda", generator=g) - 0.5
    c0 = torch.rand(3 * sc + m * ldc, device="cuda", generator=g) - 0.5
    c = c0.clone()

    def call(ta=0, tb=0, m=m, n=n, k=k, alpha=1.0, sa=m * k, sb=k * n, beta=0.5, sc=sc, pbias=bias.data_ptr(), sbias=n, mode=COL,
             act=RELU, batch=batch, pa=a.data_ptr(), pb=b.data_ptr(), pc=c.data_ptr(), lda=k, ldb=n):
        h.sgemm_batched_ex(ta, tb, m, n, k, alpha, pa, lda, sa, pb, ldb, sb, beta, pc, ldc, sc, batch, pbias, sbias, mode, act, s)

    def bits(x):
        return x.view(torch.int32)

    h.set_kernel("auto")
    # batch 0 (null operands allowed; a bias mode still wants its pointer), m 0, n 0: nothing launched
    call(batch=0, pa=0, pb=0, pc=0)
    call(batch=0, pa=0, pb=0, pc=0, pbias=0, mode=NONE)
    call(m=0)
    call(n=0)
    torch.cuda.synchronize()
    assert torch.equal(bits(c), bits(c0))
    # k == 0: the formula with s = +0 through the naive kernel -- A and B are not read (NULL), the gaps are never written
    inside = torch.zeros(c.shape, dtype=torch.bool, device="cuda")
    for i in range(batch):
        inside[i * sc:i * sc + m * ldc].view(m, ldc)[:, :n] = True
    c0_h, bias_h = c0.cpu().numpy(), bias.cpu().numpy()
    zero = np.zeros((m, n), np.float32)
    for kern in ("auto", "mfma_64x64_dma5", "naive"):
        h.set_kernel(kern)
        c.copy_(c0)
        call(k=0, alpha=-2.0, pa=0, pb=0, lda=1, sa=0, sb=0)
        assert H.last_launch().startswith(NAIVE_HEAD), H.last_launch()
        torch.cuda.synchronize()
        got = c.cpu().numpy()
        for i in range(batch):
            before = c0_h[i * sc:i * sc + m * ldc].reshape(m, ldc)[:, :n]
            want = expected(zero, -2.0, 0.5, before, bias_h[i * n:(i + 1) * n], COL, RELU)
            assert same_bits(got[i * sc:i * sc + m * ldc].reshape(m, ldc)[:, :n], want), (kern, i)
        assert torch.equal(bits(c)[~inside], bits(c0)[~inside]), kern
    # refusals: nothing launched, C untouched
    h.set_kernel("auto")
    c.copy_(c0)
    bad = [
        dict(sc=(m - 1) * ldc + n - 1, status=H.ERR_INVALID_ARG),   # C matrices overlap by one element
        dict(sc=0, status=H.ERR_INVALID_ARG),
        dict(sa=-1, status=H.ERR_INVALID_ARG),
        dict(sb=-1, status=H.ERR_INVALID_ARG),
        dict(batch=-1, status=H.ERR_INVALID_ARG),
        dict(ta=2, status=H.ERR_INVALID_ARG),
        dict(tb=-1, status=H.ERR_INVALID_ARG),
        dict(mode=3, status=H.ERR_INVALID_ARG),
        dict(mode=-1, status=H.ERR_INVALID_ARG),
        dict(act=2, status=H.ERR_INVALID_ARG),
        dict(pbias=0, status=H.ERR_INVALID_ARG),                    # a bias mode without a bias
        dict(sbias=-1, status=H.ERR_INVALID_ARG),
        dict(mode=ROW, sbias=-m, status=H.ERR_INVALID_ARG),
        dict(kernel="mfma", status=H.ERR_UNSUPPORTED),
        dict(kernel="mfma_96x96_dma5", status=H.ERR_UNSUPPORTED),
        dict(kernel="mfma_64x64_dma", status=H.ERR_UNSUPPORTED),
    ]
    for case in bad:
        case = dict(case)
        status = case.pop("status")
        h.set_kernel(case.pop("kernel", "auto"))
        with pytest.raises(H.MMultError) as e:
            call(**case)
        assert e.value.status == status, case
    h.set_kernel("auto")
    call(mode=NONE, pbias=0, sbias=-5, k=0, beta=1.0, act=0, pa=0, pb=0, lda=1)   # no bias mode: pointer and stride are ignored
    torch.cuda.synchronize()
    assert torch.equal(bits(c), bits(c0))   # (+0 + 1 * c = c)


# ---- the Python layer -------------------------------------------------------------------------------------------------
def _chains(oracle, a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return [oracle.ref_mmult(np.ascontiguousarray(a[i]), np.ascontiguousarray(b[i]), fma=True) for i in range(a.shape[0])]


def test_baddbmm(h, oracle):
    import torch
    import how_to_optimize_gemm_amd as H
    h.set_kernel("auto")
    g = torch.Generator(device="cuda").manual_seed(9)
    batch, m, n, k = 6, 70, 90, 45
    a = torch.rand((batch, m, k), device="cuda", generator=g) - 0.5
    b = torch.rand((batch, k, n), device="cuda", generator=g) - 0.5
    inp = torch.rand((batch, m, n), device="cuda", generator=g) - 0.5
    s = _chains(oracle, a, b)
    inp_h = inp.cpu().numpy()

    def want(alpha, beta, c, chains=s):
        return np.stack([expected(chains[i], alpha, beta, None if c is None else c[i], None, NONE, 0) for i in range(batch)])

    # copy first: input is left alone, out is new
    out = h.baddbmm(inp, a, b, beta=0.5, alpha=-1.3)
    assert out is not inp and same_bits(out.cpu().numpy(), want(-1.3, 0.5, inp_h)) and same_bits(inp.cpu().numpy(), inp_h)
    assert H.last_launch().endswith(", operands NN, epilogue alpha beta, batch 6"), H.last_launch()
    # in place
    x = inp.clone()
    assert h.baddbmm(x, a, b, beta=0.5, alpha=-1.3, out=x) is x and same_bits(x.cpu().numpy(), want(-1.3, 0.5, inp_h))
    # beta == 0: input is neither copied nor read
    nan = torch.full((batch, m, n), float("nan"), device="cuda")
    assert same_bits(h.baddbmm(nan, a, b, beta=0, alpha=0.7).cpu().numpy(), want(0.7, 0.0, None))
    # a broadcast input goes through out.copy_
    row = torch.rand((m, 1), device="cuda", generator=g)
    assert same_bits(h.baddbmm(row, a, b, beta=2.0).cpu().numpy(), want(1.0, 2.0, np.broadcast_to(row.cpu().numpy(), (batch, m, n))))
    # (n,) and (batch, 1, n) with beta == 1: the kernel's column bias, one launch and no copy
    v = torch.rand(n, device="cuda", generator=g) - 0.5
    vb = torch.rand((batch, 1, n + 3), device="cuda", generator=g)[:, :, :n] - 0.5   # stride(0) = n + 3
    for bias, per in ((v, lambda i: v.cpu().numpy()), (vb, lambda i: vb[i, 0].cpu().numpy())):
        got = h.baddbmm(bias, a, b, alpha=0.7)
        assert H.last_launch().endswith(", operands NN, epilogue alpha bias(col), batch 6"), H.last_launch()
        assert same_bits(got.cpu().numpy(), np.stack([expected(s[i], 0.7, 0.0, None, per(i), COL, 0) for i in range(batch)]))
    # transposed and expanded views, out as a strided window
    at = a.transpose(1, 2).contiguous().transpose(1, 2)
    b1 = b[:1].expand(batch, k, n)
    s1 = _chains(oracle, a, b1)
    big = torch.full((batch, m + 3, n + 5), float("nan"), device="cuda")
    big[:, :m, :n] = inp
    h.baddbmm(big[:, :m, :n], at, b1.transpose(1, 2).contiguous().transpose(1, 2), beta=0.5, out=big[:, :m, :n])
    assert ", operands TT," in H.last_launch(), H.last_launch()
    assert same_bits(big[:, :m, :n].cpu().numpy(), want(1.0, 0.5, inp_h, s1))
    assert bool(big[:, m:, :].isnan().all()) and bool(big[:, :, n:].isnan().all())
    assert h.baddbmm(inp[:0], a[:0], b[:0]).shape == (0, m, n)
    # errors
    for call in (lambda: h.baddbmm(inp, a[0], b[0]),
                 lambda: h.baddbmm(inp, a, b[:, :k - 1]),
                 lambda: h.baddbmm(inp[:, :, :n - 1], a, b),
                 lambda: h.baddbmm(torch.rand(n + 1, device="cuda"), a, b),
                 lambda: h.baddbmm(inp, a.double(), b.double()),
                 lambda: h.baddbmm(inp, a, b, out=torch.empty((1, m, n), device="cuda").expand(batch, m, n)),
                 lambda: h.baddbmm(inp, a.cpu(), b.cpu(), out=inp.cpu())):
        with pytest.raises(H.MMultError) as e:
            call()
        assert e.value.status == H.ERR_INVALID_ARG
    # a refused call copies nothing into its `out` first (the front end's fuzz found the copy ahead of the operands' checks)
    kept = torch.full((batch, m, n), float("nan"), device="cuda")
    for call in (lambda: h.baddbmm(inp, a, b[:, :k - 1], beta=0.5, out=kept), lambda: h.baddbmm(inp, a[:2], b, beta=0.5, out=kept),
                 lambda: h.baddbmm(inp, a, b.cpu(), out=kept), lambda: h.baddbmm(inp, a[:, :, ::2], b[:, :(k + 1) // 2], out=kept)):
        with pytest.raises(H.MMultError) as e:
            call()
        assert e.value.status == H.ERR_INVALID_ARG
    assert bool(kept.isnan().all())


def test_batched_linear(h, oracle):
    import torch
    import how_to_optimize_gemm_amd as H
    h.set_kernel("auto")
    g = torch.Generator(device="cuda").manual_seed(10)
    batch, rows, fin, fout = 5, 33, 48, 70
    x = torch.rand((batch, rows, fin), device="cuda", generator=g) - 0.5
    w = torch.rand((batch, fout, fin), device="cuda", generator=g) - 0.5
    bias = torch.rand((batch, fout), device="cuda", generator=g) - 0.5
    s = _chains(oracle, x, w.transpose(1, 2))
    s0 = _chains(oracle, x, w[:1].expand(batch, fout, fin).transpose(1, 2))

    def want(chains, bias_of, act):
        return np.stack([expected(chains[i], 1.0, 0.0, None, bias_of(i), NONE if bias_of(i) is None else COL, act) for i in range(batch)])

    bias_h = bias.cpu().numpy()
    y = h.batched_linear(x, w, bias, "relu")
    assert H.last_launch().endswith(", operands NT, epilogue bias(col) relu, batch 5"), H.last_launch()
    assert same_bits(y.cpu().numpy(), want(s, lambda i: bias_h[i], RELU))
    assert same_bits(h.batched_linear(x, w).cpu().numpy(), want(s, lambda i: None, 0))
    # a shared weight (stride 0) and a shared bias: x and y are packed, so the batch IS one layer of batch x rows rows
    y = h.batched_linear(x, w[0], bias[0], "relu")
    assert H.last_launch().endswith(f", operands NT, epilogue bias(col) relu, batch 5 folded into one {batch * rows}-row GEMM"), H.last_launch()
    assert same_bits(y.cpu().numpy(), want(s0, lambda i: bias_h[0], RELU))
    # a shared weight with a bias per matrix: one launch
    y = h.batched_linear(x, w[0], bias, "relu")
    assert H.last_launch().startswith(TILE_HEAD) and H.last_launch().endswith(", operands NT, epilogue bias(col) relu, batch 5"), H.last_launch()
    assert same_bits(y.cpu().numpy(), want(s0, lambda i: bias_h[i], RELU))
    out = torch.full((batch, rows + 1, fout + 2), float("nan"), device="cuda")
    assert same_bits(h.batched_linear(x, w, bias, out=out[:, :rows, :fout]).cpu().numpy(), want(s, lambda i: bias_h[i], 0))
    assert bool(out[:, rows:, :].isnan().all()) and bool(out[:, :, fout:].isnan().all())
    # no output feature: a bias of no floats has the address NULL and nothing to add (found by the front end's fuzz)
    assert h.batched_linear(x, w[:, :0], bias[:, :0], "relu").shape == (batch, rows, 0)
    assert h.batched_linear(x, w[0, :0], bias[0, :0]).shape == (batch, rows, 0)
    for call in (lambda: h.batched_linear(x, w, bias, "gelu"),
                 lambda: h.batched_linear(x[0], w),
                 lambda: h.batched_linear(x, w[:2]),
                 lambda: h.batched_linear(x, w, bias[:, :fout - 1]),
                 lambda: h.batched_linear(x, w, bias[:2]),
                 lambda: h.batched_linear(x, w[:, :, :fin - 1])):
        with pytest.raises(H.MMultError) as e:
            call()
        assert e.value.status == H.ERR_INVALID_ARG


# ---- graph capture ----------------------------------------------------------------------------------------------------
def test_a_captured_one_launch_call_replays_the_eager_bits(h):
    import torch
    import how_to_optimize_gemm_amd as H
    h.set_kernel("auto")
    batch, m = 64, 256
    a = torch.rand((batch, m, m), device="cuda") - 0.5
    w = torch.rand((batch, m, m), device="cuda") - 0.5
    bias = torch.rand((batch, m), device="cuda") - 0.5
    eager = h.batched_linear(a, w, bias, "relu")
    torch.cuda.synchronize()
    assert H.last_launch().startswith(TILE_HEAD) and H.last_launch().endswith(", batch 64"), H.last_launch()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    h.reserve_stream(side.cuda_stream, m, m, m)
    c = torch.full((batch, m, m), float("nan"), device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            h.batched_linear(a, w, bias, "relu", out=c)
    for rep in range(2):
        c.fill_(float("nan"))
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(c.view(torch.int32), eager.view(torch.int32)), rep
