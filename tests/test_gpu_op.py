"""Transposed operands on the GPU (mmh_sgemm_op, csrc/launch_op.hip): C = op(A) op(B) for NT, TN and TT, the transposed
operand read in place by the K2W tiles (its LDS image is the other operand's: csrc/sgemm_dma5.hpp, OP).  The contract
is NN's: every element one fp32 fma chain over ascending k -- the oracle's fused loop on the materialised operands, bit
for bit -- on AUTO and on the 64x64 / 128x64 / 128x128 tiles forced, plain and chained stream-K, whole and guarded."""
import os

import numpy as np
import pytest

from gpu_operands import _nan_stored, dev, handle_fixture, stored
from kernel_tables import FAMILY
from kernel_tables import OP_SHAPES as SHAPES

pytestmark = pytest.mark.gpu
h = handle_fixture()

OPS = {"NT": (0, 1), "TN": (1, 0), "TT": (1, 1)}
KERNELS = ["auto", "mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5"]


def tol(k):
    return 2e-7 * k + 1e-6


def run_op(h, ta, tb, a, b, c=None, accumulate=False):
    """C = op(A) op(B) for the logical (m, k) / (k, n) host arrays a, b, their stored forms dense on the device."""
    import torch
    m, k = a.shape
    n = b.shape[1]
    sa, sb = dev(stored(a, ta)), dev(stored(b, tb))
    out = torch.empty((m, n), device="cuda") if c is None else dev(c)
    h.sgemm_op(ta, tb, m, n, k, sa.data_ptr(), m if ta else k, sb.data_ptr(), k if tb else n, out.data_ptr(), n, accumulate,
               torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_op_forms_are_the_fused_chain(h, oracle, m, n, k):
    import how_to_optimize_gemm_amd as H
    a, b = oracle.harness_inputs(m, n, k, seed=m + 7 * n + 13 * k)
    want = oracle.ref_mmult(a, b, fma=True)
    checked_tol = False
    # plain and chained stream-K: the forced tiles with stream-K off and "whenever ragged" on the shapes that have rounds
    sk_modes = (1, 0, 2) if m >= 1024 else (1,)
    for kernel in KERNELS:
        h.set_kernel(kernel)
        for sk in (sk_modes if kernel != "auto" else (1,)):
            h.set_streamk(sk)
            for name, (ta, tb) in OPS.items():
                got = run_op(h, ta, tb, a, b)
                launched = H.last_launch()
                assert launched.endswith(", operands " + name), launched
                assert launched.startswith(("sgemm_mfma_dma5_op_kernel<", "sgemm_dma5_op_streamk_kernel<")), launched
                if kernel != "auto":
                    assert FAMILY[kernel] in launched, (kernel, launched)
                if sk == 0:
                    assert "persistent" not in launched, launched
                assert np.array_equal(got, want), (m, n, k, kernel, sk, name, float(np.abs(got - want).max()), launched)
                if not checked_tol:
                    assert oracle.compare_matrices(got, oracle.ref_mmult(a, b, fma=False))[0] <= tol(k)
                    checked_tol = True
    h.set_streamk(1)
    h.set_kernel("auto")


def test_stream_k_op_launches_happen(h, oracle):
    """2176^3 on the 64x64 tile under "stream-K whenever ragged" is a persistent chained launch in every op form."""
    import how_to_optimize_gemm_amd as H
    m = n = k = 2176
    a, b = oracle.harness_inputs(m, n, k, seed=5)
    h.set_kernel("mfma_64x64_dma5")
    h.set_streamk(2)
    try:
        nn = dev(np.zeros((m, n), np.float32))
        for name, (ta, tb) in OPS.items():
            got = run_op(h, ta, tb, a, b)
            launched = H.last_launch()
            assert "sgemm_dma5_op_streamk_kernel<64,64>" in launched and "persistent" in launched, launched
            if name == "NT":
                nn = got
            assert np.array_equal(got, nn)
        assert np.array_equal(nn, oracle.ref_mmult(a, b, fma=True))
        assert h.streamk_timeouts() == 0
    finally:
        h.set_streamk(1)
        h.set_kernel("auto")


@pytest.mark.parametrize("kernel", KERNELS)
def test_k_tails_padding_alignment_and_accumulate(h, oracle, kernel):
    """k in {1, 31, 33, 127}: the K tail's garbage (NaN padding past each stored row, NaN behind the last row) never
    reaches C.  Odd leading dimensions and bases one float off; accumulate onto a pre-filled C whose NaN padding (ldc > n)
    stays NaN, bit for bit."""
    import torch
    h.set_kernel(kernel)
    rng = np.random.default_rng(11)
    try:
        for k in (1, 31, 33, 127):
            for (m, n) in ((70, 150), (130, 66), (257, 129)):
                a = rng.uniform(-1, 1, (m, k)).astype(np.float32)
                b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
                c0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
                for name, (ta, tb) in OPS.items():
                    for odd in (False, True):
                        sa, sb = stored(a, ta), stored(b, tb)
                        lda = sa.shape[1] + (3 if odd else 4)
                        ldb = sb.shape[1] + (5 if odd else 8)
                        off = 1 if odd else 0
                        _, av = _nan_stored(sa.shape[0], sa.shape[1], lda, off)
                        _, bv = _nan_stored(sb.shape[0], sb.shape[1], ldb, off)
                        av[:, :sa.shape[1]] = dev(sa)
                        bv[:, :sb.shape[1]] = dev(sb)
                        for acc in (False, True):
                            ldc = n + 3
                            cflat, cv = _nan_stored(m, n, ldc, off)
                            cv[:, :n] = dev(c0)
                            h.sgemm_op(ta, tb, m, n, k, av.data_ptr(), lda, bv.data_ptr(), ldb, cv.data_ptr(), ldc, acc,
                                       torch.cuda.current_stream().cuda_stream)
                            got = cv[:, :n].cpu().numpy()
                            want = oracle.ref_mmult(a, b, c0.copy() if acc else None, fma=True)
                            assert np.array_equal(got, want), (kernel, name, m, n, k, odd, acc)
                            assert bool(torch.isnan(cv[:, n:]).all()) and bool(torch.isnan(cflat[:off]).all())
    finally:
        h.set_kernel("auto")


def test_empty_sizes(h):
    import torch
    import how_to_optimize_gemm_amd as H
    s = torch.cuda.current_stream().cuda_stream
    a = torch.rand(64 * 64, device="cuda")
    for ta, tb in OPS.values():
        c = torch.full((8, 9), 3.0, device="cuda")
        h.sgemm_op(ta, tb, 8, 9, 0, a.data_ptr(), 8, a.data_ptr(), 9, c.data_ptr(), 9, True, s)
        assert bool((c == 3.0).all())
        h.sgemm_op(ta, tb, 8, 9, 0, a.data_ptr(), 8, a.data_ptr(), 9, c.data_ptr(), 9, False, s)
        assert bool((c == 0.0).all())
        c.fill_(5.0)
        h.sgemm_op(ta, tb, 0, 9, 4, a.data_ptr(), 4, a.data_ptr(), 9, c.data_ptr(), 9, False, s)
        h.sgemm_op(ta, tb, 8, 0, 4, a.data_ptr(), 8, a.data_ptr(), 4, c.data_ptr(), 9, False, s)
        torch.cuda.synchronize()
        assert bool((c == 5.0).all())
    assert H.OP_N == 0 and H.OP_T == 1


def test_all_25_sizes_on_auto_match_the_nn_launch(h):
    """The 25 reference sizes x {NT, TN, TT} on AUTO: bit-equal to the NN AUTO launch on the materialised transposes (which
    the parity suite pins to the oracle)."""
    import torch
    h.set_kernel("auto")
    s = torch.cuda.current_stream().cuda_stream
    for n in range(1024, 4097, 128):
        g = torch.Generator(device="cuda").manual_seed(n)
        a = torch.rand((n, n), device="cuda", generator=g) - 0.5
        b = torch.rand((n, n), device="cuda", generator=g) - 0.5
        at, bt = a.t().contiguous(), b.t().contiguous()
        want = torch.empty((n, n), device="cuda")
        h.sgemm(n, n, n, a.data_ptr(), n, b.data_ptr(), n, want.data_ptr(), n, False, s)
        for name, (ta, tb) in OPS.items():
            c = torch.full((n, n), float("nan"), device="cuda")
            h.sgemm_op(ta, tb, n, n, n, (at if ta else a).data_ptr(), n, (bt if tb else b).data_ptr(), n, c.data_ptr(), n, False, s)
            assert torch.equal(c, want), (n, name)


def test_op_form_fuzz_against_the_naive_op_kernel():
    """tools/fuzz.py --ops: random shapes, leading dimensions, misaligned bases and accumulate flags on NT / TN / TT, AUTO
    and the three tiles plain and stream-K, each bit-equal (signed zeros included) to sgemm_naive_op_kernel, with NaN in
    every operand's padding and nothing written outside C's window."""
    import subprocess
    import sys
    from conftest import REPO
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "fuzz.py"), "--ops", "60", "0", "2027"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "fuzz --ops: 60 cases x 8 variants, 0 failures" in r.stdout, r.stdout[-500:]


def test_refusals_leave_c_untouched(h):
    import torch
    import how_to_optimize_gemm_amd as H
    s = torch.cuda.current_stream().cuda_stream
    m, n, k = 256, 192, 128
    a = torch.rand((k, m), device="cuda")
    b = torch.rand((n, k), device="cuda")
    for kernel in ("valu", "mfma_96x64_dma5", "mfma", "mfma_160x160_dma5", "mfma_128x64_dma"):
        h.set_kernel(kernel)
        c = torch.full((m, n), 7.0, device="cuda")
        with pytest.raises(H.MMultError) as e:
            h.sgemm_op(1, 1, m, n, k, a.data_ptr(), m, b.data_ptr(), k, c.data_ptr(), n, False, s)
        assert e.value.status == H.ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((c == 7.0).all()), kernel
    h.set_kernel("auto")
    c = torch.full((m, n), 7.0, device="cuda")
    for (ta, tb, lda, ldb) in ((1, 0, k, n), (0, 1, k, n - 100), (1, 1, m - 1, k), (0, 0, k - 1, n), (2, 0, m, n)):
        with pytest.raises(H.MMultError) as e:
            h.sgemm_op(ta, tb, m, n, k, a.data_ptr(), lda, b.data_ptr(), ldb, c.data_ptr(), n, False, s)
        assert e.value.status == H.ERR_INVALID_ARG, (ta, tb, lda, ldb)
    torch.cuda.synchronize()
    assert bool((c == 7.0).all())


def test_torch_matmul_takes_transposed_views(h):
    import torch
    import how_to_optimize_gemm_amd as H
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = torch.rand((300, 200), device="cuda") - 0.5
        w = torch.rand((150, 200), device="cuda") - 0.5
        big = torch.rand((260, 333), device="cuda") - 0.5
        w2 = torch.rand((150, 260), device="cuda") - 0.5
        a, b = big[:, 10:310], big[:, 20:170]          # row-strided windows: a.t() is (300 x 260) with stride (1, 333)
        cases = [(x, w.t()), (a.t(), b), (a.t(), w2.t()), (x, big[:200, 7:157]), (a.t(), big[:, 100:101]), (big[3:4, :260], w2.t())]
        for (p, q) in cases:
            got = h.matmul(p, q)
            want = h.matmul(p.contiguous(), q.contiguous())
            torch.cuda.synchronize()
            assert torch.equal(got, want), (p.stride(), q.stride())
        got = h.matmul(a.t(), w2.t())
        assert "operands TT" in H.last_launch(), H.last_launch()
        with pytest.raises(H.MMultError):
            h.matmul(x[:, ::2], w[:100].t())               # no unit stride
        with pytest.raises(H.MMultError):
            h.matmul(x, torch.rand(200, device="cuda").expand(150, 200).t())   # overlapping columns
        with pytest.raises(H.MMultError):
            h.matmul(x, w.t(), out=torch.empty((150, 300), device="cuda").t())   # out stays row-major
    torch.cuda.synchronize()


def test_a_captured_stream_k_op_launch_replays_the_eager_bits(h, oracle):
    import torch
    import how_to_optimize_gemm_amd as H
    m, n, k = 2304, 2176, 320
    a, b = oracle.harness_inputs(m, n, k, seed=77)
    sa, sb = dev(stored(a, 1)), dev(stored(b, 1))
    h.set_kernel("mfma_128x128_dma5")
    h.set_streamk(2)
    try:
        eager = torch.empty((m, n), device="cuda")
        s0 = torch.cuda.current_stream().cuda_stream
        h.sgemm_op(1, 1, m, n, k, sa.data_ptr(), m, sb.data_ptr(), k, eager.data_ptr(), n, False, s0)
        assert "sgemm_dma5_op_streamk_kernel<128,128>" in H.last_launch() and "persistent" in H.last_launch(), H.last_launch()
        assert np.array_equal(eager.cpu().numpy(), oracle.ref_mmult(a, b, fma=True))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        h.reserve_stream(side.cuda_stream, m, n, k)
        c = torch.full((m, n), float("nan"), device="cuda")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                h.sgemm_op(1, 1, m, n, k, sa.data_ptr(), m, sb.data_ptr(), k, c.data_ptr(), n, False, side.cuda_stream)
        for rep in range(2):
            c.fill_(float("nan"))
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(c, eager), rep
        assert h.streamk_timeouts() == 0
    finally:
        h.set_streamk(1)
        h.set_kernel("auto")


def test_op_forms_run_near_nn_rate_at_4096(h):
    """A loose floor (a conflict-ridden image or a silent fallback would be far below it): each op form at >= 0.90 of NN,
    interleaved bursts of mmh_time_sgemm_op in one process."""
    import torch
    n = 4096
    h.set_kernel("auto")
    s = torch.cuda.current_stream().cuda_stream
    a = torch.rand((n, n), device="cuda") - 0.5
    b = torch.rand((n, n), device="cuda") - 0.5
    c = torch.empty((n, n), device="cuda")
    forms = {"NN": (0, 0)} | OPS
    ms = {f: [] for f in forms}
    for f, (ta, tb) in forms.items():
        h.time_sgemm_op(ta, tb, n, n, n, a.data_ptr(), n, b.data_ptr(), n, c.data_ptr(), n, 3, 3, s)
    for _ in range(5):
        for f, (ta, tb) in forms.items():
            ms[f].append(h.time_sgemm_op(ta, tb, n, n, n, a.data_ptr(), n, b.data_ptr(), n, c.data_ptr(), n, 0, 10, s))
    best = {f: min(v) for f, v in ms.items()}
    for f in OPS:
        assert best["NN"] / best[f] >= 0.90, (f, best)
