"""The fused epilogue on the GPU (mmh_sgemm_ex, csrc/launch_ex.hip, csrc/sgemm_dma5.hpp EP):
C = act(alpha op(A) op(B) + beta C + bias) in one launch, every rounding defined (include/mmult_hip.h).

The expectation (tests/ex_ref.py) is built from the pinned oracle and numpy alone, never from the library: s = the oracle's fused chain,
then float32 numpy operations one at a time -- each rounds once, which is the contract.  32-bit patterns are compared
wherever the expectation is not NaN (and there the result must be NaN too); with the inputs below the expectation has no
NaN except in the one case that feeds NaN through beta != 0 on purpose.

tests/test_gpu_ex_parity.py::EX_INSTANTIATIONS pins each of the 48 `ex` instantiations by name and runs the special values
of the contract (inf, -0, NaN through ReLU, alpha == 0).  sgemm_naive_ex_kernel shares dma5_epilogue_apply with the tiles:
for the epilogue the numpy expectation is the only independent reference."""
import os

import numpy as np
import pytest

from bitcmp import bits_equal_on_device, first_difference, same_bits
from ex_ref import COL, NONE, RELU, ROW, expected
from gpu_operands import _nan_stored, dev, handle_fixture, stored
from kernel_tables import FAMILY, OPS
from kernel_tables import OP_SHAPES as SHAPES

pytestmark = pytest.mark.gpu
h = handle_fixture(check_timeouts=True)

KERNELS = ["auto", "mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5"]
# name: alpha, beta, bias mode, activation, C pre-filled with NaN (beta == 0 must not read it)
EPILOGUES = {
    "identity": (1.0, 0.0, NONE, 0, False),
    "alpha": (0.7, 0.0, NONE, 0, False),
    "beta_one": (1.0, 1.0, NONE, 0, False),
    "all": (-1.3, 0.5, COL, RELU, False),
    "row_bias": (1.0, 0.0, ROW, 0, False),
    "col_bias_relu_over_nan": (1.0, 0.0, COL, RELU, True),
}
# the naive kernel runs every case up to this many multiply-adds (its TN / TT loads are not coalesced)
NAIVE_MAX = 2176 ** 3


def tol(k):
    return 2e-7 * k + 1e-6


def is_ex_launch(launched, name):
    return launched.startswith(("sgemm_mfma_dma5_ex_kernel<", "sgemm_dma5_ex_streamk_kernel<")) and \
        (", operands " + name + ", epilogue") in launched


def _inputs(oracle, m, n, k, seed, scale=1.0):
    a, b = oracle.harness_inputs(m, n, k, seed=seed)
    rng = np.random.default_rng(seed)
    c0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    bias_n = rng.uniform(-1, 1, n).astype(np.float32)
    bias_m = rng.uniform(-1, 1, m).astype(np.float32)
    if scale != 1.0:
        a, b = (a * np.float32(scale)).astype(np.float32), (b * np.float32(scale)).astype(np.float32)
        c0, bias_n, bias_m = c0 * np.float32(scale * scale), bias_n * np.float32(scale * scale), bias_m * np.float32(scale * scale)
    return a, b, c0, bias_n, bias_m


def _check_shape(h, oracle, m, n, k, a, b, c0, bias_n, bias_m, epilogues, kernels):
    """Every epilogue x kernel x stream-K mode x op pair of one shape against the numpy expectation, bit for bit (compared on
    the device; a mismatch is restated on the host for the message)."""
    import torch
    import how_to_optimize_gemm_amd as H
    stream = torch.cuda.current_stream().cuda_stream
    s = oracle.ref_mmult(a, b, fma=True)
    sa = {t: dev(stored(a, t)) for t in (0, 1)}
    sb = {t: dev(stored(b, t)) for t in (0, 1)}
    bias_dev = {NONE: None, COL: dev(bias_n), ROW: dev(bias_m)}
    c0_dev = dev(c0)
    out = torch.empty((m, n), device="cuda")
    plain_out = torch.empty((m, n), device="cuda")
    sk_modes = (1, 0, 2) if m >= 1024 else (1,)
    runs = 0
    try:
        for ename, (alpha, beta, mode, act, nan_c) in epilogues.items():
            bias = {NONE: None, COL: bias_n, ROW: bias_m}[mode]
            want = expected(s, alpha, beta, c0, bias, mode, act)
            assert not np.isnan(want).any(), ename
            want_dev = dev(want)
            if ename == "identity":
                assert same_bits(want, s)   # (1 * s = s: the identity's expectation IS the oracle's chain)
            for kernel in kernels:
                if kernel == "naive" and m * n * k > NAIVE_MAX:
                    continue
                h.set_kernel(kernel)
                for sk in (sk_modes if kernel not in ("auto", "naive") else (1,)):
                    h.set_streamk(sk)
                    for name, (ta, tb) in OPS.items():
                        if nan_c:
                            out.fill_(float("nan"))
                        else:
                            out.copy_(c0_dev)
                        h.sgemm_ex(ta, tb, m, n, k, alpha, sa[ta].data_ptr(), m if ta else k, sb[tb].data_ptr(), k if tb else n, beta,
                                   out.data_ptr(), n, bias_dev[mode].data_ptr() if mode else 0, mode, act, stream)
                        launched = H.last_launch()
                        runs += 1
                        if kernel == "naive":
                            assert launched.startswith("sgemm_naive_ex_kernel"), launched
                        else:
                            assert is_ex_launch(launched, name), launched
                            if kernel != "auto":
                                assert FAMILY[kernel] in launched, (kernel, launched)
                            if sk == 0:
                                assert "persistent" not in launched, launched
                        if not bits_equal_on_device(out, want_dev):
                            got = out.cpu().numpy()
                            assert same_bits(got, want), (m, n, k, ename, kernel, sk, name, first_difference(got, want), launched)
                        if ename == "identity":
                            # ... and mmh_sgemm_op's output, bit for bit (a wrong sgemm_op does not excuse a wrong ex: the oracle above)
                            h.sgemm_op(ta, tb, m, n, k, sa[ta].data_ptr(), m if ta else k, sb[tb].data_ptr(), k if tb else n,
                                       plain_out.data_ptr(), n, False, stream)
                            assert bits_equal_on_device(out, plain_out), (m, n, k, kernel, sk, name, launched, H.last_launch())
    finally:
        h.set_streamk(1)
        h.set_kernel("auto")
    return runs


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_every_epilogue_is_the_contract_bit_for_bit(h, oracle, m, n, k):
    a, b, c0, bias_n, bias_m = _inputs(oracle, m, n, k, seed=m + 7 * n + 13 * k)
    runs = _check_shape(h, oracle, m, n, k, a, b, c0, bias_n, bias_m, EPILOGUES, KERNELS + ["naive"])
    assert runs >= len(EPILOGUES) * 4 * (4 if m * n * k > NAIVE_MAX else 5)
    got = oracle.compare_matrices(oracle.ref_mmult(a, b, fma=True), oracle.ref_mmult(a, b, fma=False))[0]
    assert got <= tol(k)


def test_a_partly_subnormal_result(h, oracle):
    """Operands scaled by 2^-62: the products sit around 2^-126, so a part of every result is subnormal, a part normal; the
    epilogue's products and sums round there as numpy's do (no flush to zero anywhere)."""
    m, n, k = 384, 320, 96
    a, b, c0, bias_n, bias_m = _inputs(oracle, m, n, k, seed=99, scale=2.0 ** -62)
    s = oracle.ref_mmult(a, b, fma=True)
    tiny = np.finfo(np.float32).tiny
    sub = (np.abs(s) < tiny) & (s != 0)
    assert sub.any() and (np.abs(s) >= tiny).any(), (int(sub.sum()), s.size)
    epi = {e: EPILOGUES[e] for e in ("identity", "alpha", "beta_one", "all", "row_bias")}
    _check_shape(h, oracle, m, n, k, a, b, c0, bias_n, bias_m, epi, KERNELS + ["naive"])


def test_stream_k_ex_launches_happen(h, oracle):
    """2176^3 on the 64x64 tile and 2304 x 2176 x 320 on the 128x128 tile under "stream-K whenever ragged" are persistent
    chained launches of the `ex` kernels in every op form -- and never with stream-K off."""
    import torch
    import how_to_optimize_gemm_amd as H
    stream = torch.cuda.current_stream().cuda_stream
    alpha, beta, mode, act, _ = EPILOGUES["all"]
    try:
        for kernel, (m, n, k) in (("mfma_64x64_dma5", (2176, 2176, 2176)), ("mfma_128x128_dma5", (2304, 2176, 320))):
            a, b, c0, bias_n, _ = _inputs(oracle, m, n, k, seed=5)
            want = dev(expected(oracle.ref_mmult(a, b, fma=True), alpha, beta, c0, bias_n, mode, act))
            sa = {t: dev(stored(a, t)) for t in (0, 1)}
            sb = {t: dev(stored(b, t)) for t in (0, 1)}
            c0_dev, bias = dev(c0), dev(bias_n)
            h.set_kernel(kernel)
            for sk in (2, 0):
                h.set_streamk(sk)
                for name, (ta, tb) in OPS.items():
                    out = c0_dev.clone()
                    h.sgemm_ex(ta, tb, m, n, k, alpha, sa[ta].data_ptr(), m if ta else k, sb[tb].data_ptr(), k if tb else n, beta,
                               out.data_ptr(), n, bias.data_ptr(), mode, act, stream)
                    launched = H.last_launch()
                    if sk == 2:
                        assert "sgemm_dma5_ex_streamk_kernel" + FAMILY[kernel] in launched and "persistent" in launched, launched
                    else:
                        assert "sgemm_mfma_dma5_ex_kernel" + FAMILY[kernel] in launched and "persistent" not in launched, launched
                    assert launched.endswith(", operands " + name + ", epilogue alpha beta bias(col) relu"), launched
                    assert bits_equal_on_device(out, want), (kernel, sk, name, launched)
        assert h.streamk_timeouts() == 0
    finally:
        h.set_streamk(1)
        h.set_kernel("auto")


@pytest.mark.parametrize("kernel", KERNELS + ["naive"])
def test_k_tails_padding_alignment_and_bias_offsets(h, oracle, kernel):
    """k in {1, 31, 33, 127}: NaN in every operand's padding and in C's (ldc > n), odd leading dimensions, bases and the bias
    one float off: results exact, the padding still NaN, nothing written in front of or behind C's window."""
    import torch
    h.set_kernel(kernel)
    rng = np.random.default_rng(11)
    stream = torch.cuda.current_stream().cuda_stream
    epis = ("all", "row_bias", "col_bias_relu_over_nan", "beta_one")
    try:
        for k in (1, 31, 33, 127):
            for (m, n) in ((70, 150), (130, 66), (257, 129)):
                a = rng.uniform(-1, 1, (m, k)).astype(np.float32)
                b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
                c0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
                bias_n = rng.uniform(-1, 1, n).astype(np.float32)
                bias_m = rng.uniform(-1, 1, m).astype(np.float32)
                s = oracle.ref_mmult(a, b, fma=True)
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
                        for ename in epis:
                            alpha, beta, mode, act, nan_c = EPILOGUES[ename]
                            bias_host = {NONE: None, COL: bias_n, ROW: bias_m}[mode]
                            bias_ptr = 0
                            if mode:
                                bflat = torch.full((off + len(bias_host) + 8,), float("nan"), device="cuda")
                                bflat[off:off + len(bias_host)] = dev(bias_host)
                                bias_ptr = bflat[off:].data_ptr()
                            ldc = n + 3
                            cflat, cv = _nan_stored(m, n, ldc, off)
                            if not nan_c:
                                cv[:, :n] = dev(c0)
                            h.sgemm_ex(ta, tb, m, n, k, alpha, av.data_ptr(), lda, bv.data_ptr(), ldb, beta, cv.data_ptr(), ldc, bias_ptr,
                                       mode, act, stream)
                            got = cv[:, :n].cpu().numpy()
                            want = expected(s, alpha, beta, c0, bias_host, mode, act)
                            assert same_bits(got, want), (kernel, name, m, n, k, odd, ename, first_difference(got, want))
                            assert not np.isnan(got).any()
                            assert bool(torch.isnan(cv[:, n:]).all()) and bool(torch.isnan(cflat[:off]).all())
                            assert bool(torch.isnan(cflat[off + m * ldc:]).all())
    finally:
        h.set_kernel("auto")


def test_beta_reads_c_and_only_beta_does(h, oracle):
    """The one case with NaN in the expectation: NaN planted in C reaches the result through beta != 0 exactly where it was
    planted -- and nowhere with beta == 0."""
    import torch
    m, n, k = 200, 136, 72
    a, b, c0, bias_n, _ = _inputs(oracle, m, n, k, seed=3)
    c0[::7, ::5] = np.nan
    s = oracle.ref_mmult(a, b, fma=True)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for kernel in KERNELS + ["naive"]:
            h.set_kernel(kernel)
            for name, (ta, tb) in OPS.items():
                sa, sb = dev(stored(a, ta)), dev(stored(b, tb))
                for (alpha, beta) in ((1.0, 0.5), (0.7, 0.0)):
                    want = expected(s, alpha, beta, c0, bias_n, COL, 0)
                    assert np.isnan(want).any() == (beta != 0)
                    out, bias = dev(c0), dev(bias_n)
                    h.sgemm_ex(ta, tb, m, n, k, alpha, sa.data_ptr(), m if ta else k, sb.data_ptr(), k if tb else n, beta, out.data_ptr(),
                               n, bias.data_ptr(), COL, 0, stream)
                    got = out.cpu().numpy()
                    assert same_bits(got, want), (kernel, name, alpha, beta, first_difference(got, want))
    finally:
        h.set_kernel("auto")


def test_empty_sizes(h):
    """k == 0: the formula with s = +0 (A and B are not read: NULL is fine), every epilogue; m == 0, n == 0: nothing happens."""
    import torch
    s = torch.cuda.current_stream().cuda_stream
    m, n = 9, 70
    rng = np.random.default_rng(2)
    c0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    bias_n, bias_m = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, m).astype(np.float32)
    zero = np.zeros((m, n), np.float32)
    try:
        for kernel in KERNELS + ["naive"]:
            h.set_kernel(kernel)
            for ta, tb in OPS.values():
                for ename, (alpha, beta, mode, act, nan_c) in EPILOGUES.items():
                    bias_host = {NONE: None, COL: bias_n, ROW: bias_m}[mode]
                    bias = dev(bias_host) if mode else None
                    out = torch.full((m, n), float("nan"), device="cuda") if nan_c else dev(c0)
                    h.sgemm_ex(ta, tb, m, n, 0, alpha, 0, max(m, 1), 0, max(n, 1), beta, out.data_ptr(), n, bias.data_ptr() if mode else 0,
                               mode, act, s)
                    want = expected(zero, alpha, beta, c0, bias_host, mode, act)
                    assert same_bits(out.cpu().numpy(), want), (kernel, ta, tb, ename)
        h.set_kernel("auto")
        a = torch.rand(64 * 64, device="cuda")
        c = torch.full((8, 9), 5.0, device="cuda")
        for ta, tb in OPS.values():
            h.sgemm_ex(ta, tb, 0, 9, 4, 2.0, a.data_ptr(), 4, a.data_ptr(), 9, 3.0, c.data_ptr(), 9, a.data_ptr(), COL, RELU, s)
            h.sgemm_ex(ta, tb, 8, 0, 4, 2.0, a.data_ptr(), 8, a.data_ptr(), 4, 3.0, c.data_ptr(), 9, a.data_ptr(), ROW, RELU, s)
        torch.cuda.synchronize()
        assert bool((c == 5.0).all())
    finally:
        h.set_kernel("auto")


def test_refusals_leave_c_untouched(h):
    import torch
    import how_to_optimize_gemm_amd as H
    s = torch.cuda.current_stream().cuda_stream
    m, n, k = 256, 192, 128
    a = torch.rand((m, m), device="cuda")   # (room for every reading of the operands, should a call not be refused)
    b = torch.rand((m, m), device="cuda")
    bias = torch.rand((m + n,), device="cuda")
    try:
        for kernel in ("valu", "mfma", "mfma_96x64_dma5", "mfma_160x160_dma5", "mfma_128x64_dma"):
            h.set_kernel(kernel)
            for (ta, tb) in ((0, 0), (1, 1)):
                c = torch.full((m, n), 7.0, device="cuda")
                with pytest.raises(H.MMultError) as e:
                    h.sgemm_ex(ta, tb, m, n, k, 0.5, a.data_ptr(), m, b.data_ptr(), max(k, n), 2.0, c.data_ptr(), n, bias.data_ptr(), COL, RELU, s)
                assert e.value.status == H.ERR_UNSUPPORTED, kernel
                torch.cuda.synchronize()
                assert bool((c == 7.0).all()), kernel
        h.set_kernel("auto")
        c = torch.full((m, n), 7.0, device="cuda")
        bad = [dict(ta=2), dict(tb=-1), dict(mode=3), dict(mode=-1), dict(act=2), dict(act=-1), dict(mode=COL, bias=0), dict(mode=ROW, bias=0),
               dict(ta=1, lda=m - 1), dict(tb=1, ldb=k - 1), dict(ldc=n - 1)]
        for case in bad:
            p = dict(ta=0, tb=0, lda=max(m, k), ldb=max(k, n), ldc=n, mode=NONE, act=0, bias=bias.data_ptr())
            p.update(case)
            with pytest.raises(H.MMultError) as e:
                h.sgemm_ex(p["ta"], p["tb"], m, n, k, 0.5, a.data_ptr(), p["lda"], b.data_ptr(), p["ldb"], 2.0, c.data_ptr(), p["ldc"],
                           p["bias"], p["mode"], p["act"], s)
            assert e.value.status == H.ERR_INVALID_ARG, case
        torch.cuda.synchronize()
        assert bool((c == 7.0).all())
    finally:
        h.set_kernel("auto")


def test_addmm_and_linear(h, oracle):
    """MMult.addmm / MMult.linear: the contract's expectation bit for bit -- contiguous and transposed-view operands,
    `out is input` and not, 1-D and 2-D `input` -- and, as a sanity check against an implementation that is not ours,
    torch.addmm / torch.nn.functional.linear (+ relu) within the project's tolerance scaled by |alpha| + |beta| + 1."""
    import torch
    import how_to_optimize_gemm_amd as H
    m, n, k = 300, 150, 200
    a, b, c0, bias_n, _ = _inputs(oracle, m, n, k, seed=21)
    s = oracle.ref_mmult(a, b, fma=True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ta_, tb_ = dev(a), dev(b)
        views = {"contiguous": (ta_, tb_), "a.t()": (dev(stored(a, 1)).t(), tb_), "b.t()": (ta_, dev(stored(b, 1)).t()),
                 "both": (dev(stored(a, 1)).t(), dev(stored(b, 1)).t())}
        for vname, (pa, pb) in views.items():
            for (alpha, beta) in ((1.0, 1.0), (0.7, -0.5), (2.0, 0.0)):
                bound = tol(k) * (abs(alpha) + abs(beta) + 1)
                # 2-D input, out=None / out given / in place
                want = expected(s, alpha, beta, c0, None, NONE, 0)
                inp = dev(c0)
                got = h.addmm(inp, pa, pb, beta=beta, alpha=alpha)
                assert same_bits(got.cpu().numpy(), want), (vname, alpha, beta, "out=None")
                assert torch.equal(inp, dev(c0))
                ref = torch.addmm(inp, pa, pb, beta=beta, alpha=alpha)
                assert float((got - ref).abs().max()) <= bound, (vname, alpha, beta)
                out = torch.full((m, n), float("nan"), device="cuda")
                assert h.addmm(inp, pa, pb, beta=beta, alpha=alpha, out=out) is out
                assert same_bits(out.cpu().numpy(), want), (vname, alpha, beta, "out")
                assert h.addmm(inp, pa, pb, beta=beta, alpha=alpha, out=inp) is inp
                assert same_bits(inp.cpu().numpy(), want), (vname, alpha, beta, "in place")
                # 1-D input: the bias path (beta == 1) or a broadcast copy
                vec = dev(bias_n)
                if beta == 1.0:
                    want1 = expected(s, alpha, 0.0, None, bias_n, COL, 0)
                else:
                    want1 = expected(s, alpha, beta, np.broadcast_to(bias_n, (m, n)), None, NONE, 0)
                got = h.addmm(vec, pa, pb, beta=beta, alpha=alpha)
                if beta == 1.0:
                    assert "bias(col)" in H.last_launch(), H.last_launch()
                assert same_bits(got.cpu().numpy(), want1), (vname, alpha, beta, "1-D")
                ref = torch.addmm(vec, pa, pb, beta=beta, alpha=alpha)
                assert float((got - ref).abs().max()) <= bound, (vname, alpha, beta, "1-D")
        # linear: w stored out x in, read in place
        x, w = dev(a), dev(stored(b, 1))
        for xname, px in (("contiguous", x), ("x view", dev(stored(a, 1)).t())):
            for act in (None, "relu"):
                for with_bias in (True, False):
                    want = expected(s, 1.0, 0.0, None, bias_n if with_bias else None, COL if with_bias else NONE, RELU if act else 0)
                    bias = dev(bias_n) if with_bias else None
                    got = h.linear(px, w, bias, activation=act)
                    launched = H.last_launch()
                    assert ("operands TT" if xname == "x view" else "operands NT") in launched, launched
                    assert ("relu" in launched) == (act is not None) and ("bias(col)" in launched) == with_bias, launched
                    assert same_bits(got.cpu().numpy(), want), (xname, act, with_bias)
                    ref = torch.nn.functional.linear(px, w, bias)
                    if act:
                        ref = torch.relu(ref)
                    assert float((got - ref).abs().max()) <= tol(k) * 2, (xname, act, with_bias)
                    out = torch.full((m, n), float("nan"), device="cuda")
                    assert h.linear(px, w, bias, activation=act, out=out) is out
                    assert same_bits(out.cpu().numpy(), want)
        with pytest.raises(H.MMultError):
            h.linear(x, w, activation="gelu")
        with pytest.raises(H.MMultError):
            h.linear(x, w, dev(bias_n)[:n - 1])
        with pytest.raises(H.MMultError):
            h.addmm(dev(c0)[:, :n - 1], ta_, tb_)
        # a refused call copies nothing into its `out` first (the front end's fuzz found the copy ahead of the checks): operands
        # whose inner dimensions disagree, an operand without a unit stride, an `out` whose rows overlap
        kept = torch.full((m + 1, n), float("nan"), device="cuda")
        for pa, pb, out in ((ta_[:, :k - 1], tb_, kept[:m]), (ta_[:, ::2], tb_[:k // 2], kept[:m]), (ta_.cpu(), tb_, kept[:m]),
                            (ta_, tb_, torch.as_strided(kept, (m, n), (n - 1, 1)))):
            with pytest.raises(H.MMultError) as e:
                h.addmm(dev(c0), pa, pb, beta=0.5, out=out)
            assert e.value.status == H.ERR_INVALID_ARG
        assert bool(kept.isnan().all())
        # no output column: a bias of no floats has the address NULL and nothing to add (found by the front end's fuzz)
        none = torch.empty((0,), device="cuda")
        assert h.linear(x, w[:0], none, activation="relu").shape == (m, 0)
        assert h.addmm(none, ta_, tb_[:, :0]).shape == (m, 0)
    torch.cuda.synchronize()


def test_a_captured_stream_k_ex_launch_replays_the_eager_bits(h, oracle):
    import torch
    import how_to_optimize_gemm_amd as H
    m, n, k = 2304, 2176, 320
    a, b, c0, bias_n, _ = _inputs(oracle, m, n, k, seed=77)
    alpha, beta, mode, act, _ = EPILOGUES["all"]
    sa, sb, bias, c0_dev = dev(stored(a, 1)), dev(stored(b, 1)), dev(bias_n), dev(c0)
    h.set_kernel("mfma_128x128_dma5")
    h.set_streamk(2)
    try:
        eager = c0_dev.clone()
        s0 = torch.cuda.current_stream().cuda_stream
        h.sgemm_ex(1, 1, m, n, k, alpha, sa.data_ptr(), m, sb.data_ptr(), k, beta, eager.data_ptr(), n, bias.data_ptr(), mode, act, s0)
        assert "sgemm_dma5_ex_streamk_kernel<128,128>" in H.last_launch() and "persistent" in H.last_launch(), H.last_launch()
        want = expected(oracle.ref_mmult(a, b, fma=True), alpha, beta, c0, bias_n, mode, act)
        assert same_bits(eager.cpu().numpy(), want)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        h.reserve_stream(side.cuda_stream, m, n, k)
        c = c0_dev.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                h.sgemm_ex(1, 1, m, n, k, alpha, sa.data_ptr(), m, sb.data_ptr(), k, beta, c.data_ptr(), n, bias.data_ptr(), mode, act,
                           side.cuda_stream)
        for rep in range(2):
            c.copy_(c0_dev)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                graph.replay()
            torch.cuda.synchronize()
            assert bits_equal_on_device(c, eager), rep
        assert h.streamk_timeouts() == 0
    finally:
        h.set_streamk(1)
        h.set_kernel("auto")


def test_ex_fuzz_against_the_naive_ex_kernel():
    """tools/fuzz.py --ex: random shapes, leading dimensions, misaligned bases and epilogues on all four op pairs, AUTO and the
    three tiles plain and stream-K, each bit-equal to sgemm_naive_ex_kernel, with NaN in every operand's padding and nothing
    written outside C's window.  (The numpy expectation above is the primary check; this widens the shapes.)"""
    import subprocess
    import sys
    from conftest import REPO
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "fuzz.py"), "--ex", "40", "0", "2028"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "fuzz --ex: 40 cases x 8 variants, 0 failures" in r.stdout, r.stdout[-500:]


def _bursts(calls, bursts=5):
    """Interleaved bursts: every callable once per round, `bursts` rounds; the best (smallest) time of each."""
    ms = {name: [] for name in calls}
    for _ in range(bursts):
        for name, fn in calls.items():
            ms[name].append(fn())
    return {name: min(v) for name, v in ms.items()}, ms


def test_bias_relu_epilogue_runs_near_the_plain_rate_at_4096(h):
    """Floor 1: C = relu(op(A) op(B) + bias) at 4096^3 on AUTO, NN and NT, takes at most 1 / 0.90 of mmh_sgemm_op on the same
    shape (best of 5 interleaved bursts of 10 calls) -- there to catch a silent fallback or a spilling kernel, not to rank the
    epilogue."""
    import torch
    n = 4096
    h.set_kernel("auto")
    s = torch.cuda.current_stream().cuda_stream
    a = torch.rand((n, n), device="cuda") - 0.5
    b = torch.rand((n, n), device="cuda") - 0.5
    bias = torch.rand((n,), device="cuda") - 0.5
    c = torch.empty((n, n), device="cuda")
    calls = {}
    for name in ("NN", "NT"):
        ta, tb = OPS[name]
        calls["op " + name] = lambda w=0, r=10, ta=ta, tb=tb: h.time_sgemm_op(ta, tb, n, n, n, a.data_ptr(), n, b.data_ptr(), n, c.data_ptr(), n, w, r, s)
        calls["ex " + name] = lambda w=0, r=10, ta=ta, tb=tb: h.time_sgemm_ex(ta, tb, n, n, n, 1.0, a.data_ptr(), n, b.data_ptr(), n, 0.0, c.data_ptr(),
                                                                              n, bias.data_ptr(), COL, RELU, w, r, s)
    for fn in calls.values():
        fn(3, 3)
    best, ms = _bursts(calls)
    print("ms per call, 4096^3:", {k_: [round(x, 4) for x in v] for k_, v in ms.items()})
    for name in ("NN", "NT"):
        ratio = best["op " + name] / best["ex " + name]
        print(f"bias + ReLU epilogue / plain op call, {name}: {ratio:.4f}")
        assert ratio >= 0.90, (name, best)


def test_fused_linear_is_no_slower_than_three_launches(h):
    """Floor 2: y = relu(x W^T + b) at 4096 x 4096 x 512 (NT) in one launch takes no longer than today's unfused sequence --
    matmul(out=y), y.add_(bias), y.relu_() on the same stream -- both timed with events around 10 repetitions, best of 5
    interleaved bursts.  No margin: the two extra passes move 256 MB behind a GEMM of about 115 us."""
    import torch
    m, n, k = 4096, 4096, 512
    h.set_kernel("auto")
    x = torch.rand((m, k), device="cuda") - 0.5
    w = torch.rand((n, k), device="cuda") - 0.5
    bias = torch.rand((n,), device="cuda") - 0.5
    y = torch.empty((m, n), device="cuda")

    def timed(step, reps=10):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            step()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / reps

    def fused():
        h.linear(x, w, bias, activation="relu", out=y)

    def unfused():
        h.matmul(x, w.t(), out=y)
        y.add_(bias)
        y.relu_()

    fused()
    got = y.clone()
    unfused()
    assert float((got - y).abs().max()) <= tol(k) * 2   # (the same layer; bits are the tests' above)
    calls = {"fused": lambda: timed(fused), "unfused": lambda: timed(unfused)}
    for fn in calls.values():
        fn()
    best, ms = _bursts(calls)
    print("ms per layer, 4096 x 4096 x 512 NT:", {k_: [round(v_, 4) for v_ in v] for k_, v in ms.items()})
    print(f"fused / unfused time: {best['fused'] / best['unfused']:.4f}")
    assert best["fused"] <= best["unfused"], best


def test_zz_no_stream_k_hand_over_timed_out(h):
    assert h.streamk_timeouts() == 0
