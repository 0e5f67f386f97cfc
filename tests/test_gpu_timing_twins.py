"""What the timing twins COMPUTE: mmh_time_sgemm, _op, _ex, _batched and _batched_ex run the call they time, so one timed
call (warmup 0, reps 1) must leave in C what the untimed call's own references say -- the oracle's fused chain
(oracle.ref_mmult, fma=True) and, for the epilogue, tests/ex_ref.py.  The twins take the longest argument lists of the ABI,
and every other test only looks at the time they return: a slip in a twin's argument order would pass them all.

One problem, chosen so that no two arguments can change places unnoticed: m, n, k = 96, 160, 72 (all different; more than one
64-wide tile each way, tile edges in both, a K tail), leading dimensions 4, 8 and 12 floats past the rows with NaN in the
padding, A stored transposed where the call has op flags, alpha = 0.75 and beta = -0.5 on a prefilled C, a ROW bias with
ReLU, and a batch of 3 whose A, B, C and bias strides are each a different amount past dense.  The whole C buffer is
compared, so a call that writes outside its windows fails too."""
import types

import numpy as np
import pytest

import ex_ref
import how_to_optimize_gemm_amd as H
from bitcmp import first_difference, same_bits
from gpu_operands import handle_fixture

pytestmark = pytest.mark.gpu

amm = handle_fixture("auto")

M, N, K, BATCH = 96, 160, 72, 3
LDA_N, LDA_T, LDB, LDC = K + 4, M + 4, N + 8, N + 12   # A stored m x k (mmh_time_sgemm) or k x m (transa = OP_T)
SA, SB, SC, SBIAS = K * LDA_T + 16, K * LDB + 24, M * LDC + 40, M + 7
ALPHA, BETA = 0.75, -0.5


def _lay(mats, ld, stride):
    """The matrices `stride` floats apart at leading dimension `ld` in one flat buffer, NaN everywhere else."""
    rows, cols = mats[0].shape
    flat = np.full((len(mats) - 1) * stride + rows * ld + 8, np.nan, np.float32)
    for i, x in enumerate(mats):
        flat[i * stride:i * stride + rows * ld].reshape(rows, ld)[:, :cols] = x
    return flat


@pytest.fixture(scope="module")
def problem(oracle):
    rng = np.random.default_rng(20261019)
    uni = lambda *shape: [rng.uniform(-1, 1, shape).astype(np.float32) for _ in range(BATCH)]
    a, b, c0, bias = uni(M, K), uni(K, N), uni(M, N), uni(1, M)
    chain = [oracle.ref_mmult(a[i], b[i], fma=True) for i in range(BATCH)]
    ex = [ex_ref.expected(chain[i], ALPHA, BETA, c0[i], bias[i][0], ex_ref.ROW, ex_ref.RELU) for i in range(BATCH)]
    assert all(0 < np.count_nonzero(x) < x.size for x in ex)   # the ReLU closes some elements and leaves others
    at = [np.ascontiguousarray(x.T) for x in a]
    return types.SimpleNamespace(
        a_n=_lay(a[:1], LDA_N, 0), a_t=_lay(at[:1], LDA_T, 0), a_ts=_lay(at, LDA_T, SA), b=_lay(b[:1], LDB, 0), bs=_lay(b, LDB, SB),
        c0=_lay(c0[:1], LDC, 0), c0s=_lay(c0, LDC, SC), bias=_lay(bias[:1], M, 0), biases=_lay(bias, M, SBIAS),
        chain=_lay(chain[:1], LDC, 0), chains=_lay(chain, LDC, SC), ex=_lay(ex[:1], LDC, 0), exs=_lay(ex, LDC, SC))


def _timed(call, want, c0, *operands):
    """call(pointers of the operands and of C, stream) -> ms on device copies; C afterwards is `want`, bit for bit."""
    import torch
    dev = [torch.from_numpy(x).cuda() for x in (*operands, c0)]
    ms = call(*(t.data_ptr() for t in dev), torch.cuda.current_stream().cuda_stream)
    got = dev[-1].cpu().numpy()
    assert ms > 0.0
    assert same_bits(got, want), (H.last_launch(), first_difference(got, want))


def test_time_sgemm_computes_the_chain(amm, problem):
    p = problem
    _timed(lambda a, b, c, s: amm.time_sgemm(M, N, K, a, LDA_N, b, LDB, c, LDC, warmup=0, reps=1, stream=s), p.chain, p.c0, p.a_n, p.b)


def test_time_sgemm_op_computes_the_chain(amm, problem):
    p = problem
    _timed(lambda a, b, c, s: amm.time_sgemm_op(H.OP_T, H.OP_N, M, N, K, a, LDA_T, b, LDB, c, LDC, warmup=0, reps=1, stream=s),
           p.chain, p.c0, p.a_t, p.b)


def test_time_sgemm_ex_computes_the_epilogue(amm, problem):
    p = problem
    _timed(lambda a, b, bias, c, s: amm.time_sgemm_ex(H.OP_T, H.OP_N, M, N, K, ALPHA, a, LDA_T, b, LDB, BETA, c, LDC, bias, H.BIAS_ROW,
                                                      H.ACT_RELU, warmup=0, reps=1, stream=s), p.ex, p.c0, p.a_t, p.b, p.bias)


def test_time_sgemm_batched_computes_every_chain(amm, problem):
    p = problem
    _timed(lambda a, b, c, s: amm.time_sgemm_batched(H.OP_T, H.OP_N, M, N, K, a, LDA_T, SA, b, LDB, SB, c, LDC, SC, BATCH, warmup=0,
                                                     reps=1, stream=s), p.chains, p.c0s, p.a_ts, p.bs)


def test_time_sgemm_batched_ex_computes_every_epilogue(amm, problem):
    p = problem
    _timed(lambda a, b, bias, c, s: amm.time_sgemm_batched_ex(H.OP_T, H.OP_N, M, N, K, ALPHA, a, LDA_T, SA, b, LDB, SB, BETA, c, LDC, SC,
                                                              BATCH, bias, SBIAS, H.BIAS_ROW, H.ACT_RELU, warmup=0, reps=1,
                                                              stream=s), p.exs, p.c0s, p.a_ts, p.bs, p.biases)
