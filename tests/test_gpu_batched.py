"""Strided batched SGEMM on the GPU (mmh_sgemm_batched, MMult.bmm; csrc/launch_batched.hip): C_i = op(A_i) op(B_i) (+ C_i)
for every matrix of a batch, matrix i at base + i * stride.  The contract is mmh_sgemm_op's, matrix by matrix: one fp32
fma chain over ascending k per element -- the oracle's fused loop, bit for bit (signed zeros included) -- on AUTO (fold,
one launch, loop), the three K2W tiles forced and the naive batched kernel; nothing outside the C matrices is written."""
import os

import numpy as np
import pytest

from bitcmp import same_bits
from gpu_operands import Batch, handle_fixture
from kernel_tables import FAMILY, OPS

pytestmark = pytest.mark.gpu
h = handle_fixture(reset_kernel=True)

KERNELS = ["auto", "mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5", "naive"]


# name: (m, n, k, batch, extra Batch arguments, AUTO's expected form marker or None)
CASES = {
    "many_small_512x64": (64, 64, 64, 512, {}, "batch 512"),
    "thin_1_15_ktail": (129, 143, 77, 3, {"ldc": 150, "sc": 129 * 150 + 40}, "batch 3"),
    "thin_16_17_ktail": (144, 145, 33, 3, {"offs": (1, 2, 3)}, "batch 3"),
    "strides_not_mult_of_4": (64, 96, 64, 5, {"sa": 64 * 64 + 1, "sb": 64 * 96 + 3, "sc": 64 * 96 + 5}, "batch 5"),
    "broadcast_a": (100, 72, 40, 6, {"sa": 0, "sc": 100 * 72 + 8}, "batch 6"),
    "broadcast_b": (72, 100, 40, 6, {"sb": 0, "sc": 72 * 100 + 8}, "batch 6"),
    "fold": (128, 128, 64, 8, {"sb": 0}, "folded into one 1024-row GEMM"),
    "loop_2x2176": (2176, 2176, 2176, 2, {}, "as a loop of 2 per-matrix launches"),
}


def _case(op, name):
    m, n, k, batch, extra, marker = CASES[name]
    ta, tb = OPS[op]
    extra = dict(extra)
    if name == "fold" and ta:
        marker = "batch 8"   # (transposed A is never folded)
    return Batch(ta, tb, m, n, k, batch, seed=sum(map(ord, name)) + 7, **extra), marker


# (the 2176^3 loop case runs on NN and TT: the op forms' per-matrix plan is test_gpu_op's)
PARAMS = [(op, name) for name in CASES for op in OPS if name != "loop_2x2176" or op in ("NN", "TT")]


@pytest.mark.parametrize("op,name", PARAMS)
def test_every_matrix_is_the_fused_chain(h, oracle, op, name):
    import how_to_optimize_gemm_amd as H
    import torch
    bt, marker = _case(op, name)
    wants = [bt.want(oracle, i, False) for i in range(bt.batch)]
    for kern in KERNELS:
        if name == "loop_2x2176" and kern == "naive":
            continue
        h.set_kernel(kern)
        got = bt.run(h)
        launch = H.last_launch()
        for i in range(bt.batch):
            assert same_bits(bt.c_window(got, i), wants[i]), (kern, op, name, i, launch)
        inside = np.zeros(got.shape, dtype=bool)
        for i in range(bt.batch):
            o = bt.offs[2] + i * bt.sc
            inside[o:o + bt.m * bt.ldc].reshape(bt.m, bt.ldc)[:, :bt.n] = True
        assert same_bits(got[~inside], bt.c0[~inside]), (kern, "wrote outside the C matrices")
        if kern == "auto":
            assert marker in launch, (marker, launch)
        elif kern == "naive":
            assert "sgemm_naive_batched_kernel" in launch and f"batch {bt.batch}" in launch, launch
        else:
            assert f"sgemm_mfma_dma5_batched_kernel{FAMILY[kern]}" in launch and f"batch {bt.batch}" in launch, launch
            if name == "strides_not_mult_of_4":
                assert "guarded" in launch, launch
    h.set_kernel("auto")
    # ... and each matrix is what mmh_sgemm_op computes on it alone
    s = torch.cuda.current_stream().cuda_stream
    for i in sorted({0, bt.batch // 2, bt.batch - 1}):
        a, b = bt.logical(i)
        sa = torch.from_numpy(np.ascontiguousarray(a.T if bt.ta else a)).cuda()
        sb = torch.from_numpy(np.ascontiguousarray(b.T if bt.tb else b)).cuda()
        c = torch.empty((bt.m, bt.n), device="cuda")
        h.sgemm_op(bt.ta, bt.tb, bt.m, bt.n, bt.k, sa.data_ptr(), bt.m if bt.ta else bt.k, sb.data_ptr(), bt.k if bt.tb else bt.n,
                   c.data_ptr(), bt.n, False, s)
        assert same_bits(c.cpu().numpy(), wants[i]), (op, name, i)


@pytest.mark.parametrize("kern", KERNELS)
def test_accumulate_gaps_and_signed_zero_on_a_k_tail(h, oracle, kern):
    h.set_kernel(kern)
    try:
        for op, (ta, tb) in OPS.items():
            bt = Batch(ta, tb, 131, 187, 77, 3, seed=11, ldc=190, sc=131 * 190 + 17, offs=(1, 0, 2))
            bt.check(oracle, bt.run(h, accumulate=True), True, (kern, op, "accumulate"))
            # -0 in C and A, B positive: every product -0, so every accumulator stays -0 -- the K tail's dead lanes included
            pos = np.random.default_rng(13)
            z = Batch(ta, tb, 131, 187, 77, 2, seed=12, sc=131 * 187 + 9, a_val=lambda r, c: np.full((r, c), -0.0, np.float32),
                      b_val=lambda r, c: pos.uniform(0.5, 1.5, (r, c)).astype(np.float32),
                      c_val=lambda r, c: np.full((r, c), -0.0, np.float32))
            got = z.run(h, accumulate=True)
            z.check(oracle, got, True, (kern, op, "signed zero"))
            assert np.signbit(z.c_window(got, 1)).all()
    finally:
        h.set_kernel("auto")


def test_empty_cases_and_refusals_leave_c_untouched(h):
    import torch
    import how_to_optimize_gemm_amd as H
    s = torch.cuda.current_stream().cuda_stream
    m, n, k, batch = 40, 50, 30, 4
    ldc, sc = 52, 40 * 52 + 7
    a = torch.rand(batch * m * k, device="cuda")
    b = torch.rand(batch * k * n, device="cuda")
    c = torch.full((3 * sc + m * ldc,), float("nan"), device="cuda")
    c0 = c.clone()
    # batch 0, m 0, n 0: nothing launched (null pointers allowed with batch 0)
    h.sgemm_batched(0, 0, m, n, k, 0, k, m * k, 0, n, k * n, 0, ldc, sc, 0, False, s)
    h.sgemm_batched(0, 0, 0, n, k, a.data_ptr(), k, m * k, b.data_ptr(), n, k * n, c.data_ptr(), ldc, sc, batch, False, s)
    h.sgemm_batched(0, 0, m, 0, k, a.data_ptr(), k, m * k, b.data_ptr(), n, k * n, c.data_ptr(), ldc, sc, batch, False, s)
    torch.cuda.synchronize()
    assert torch.equal(c.isnan(), c0.isnan()) and bool(c.isnan().all())
    # k == 0: every C matrix zeroed, the gaps and the ld padding untouched; accumulate leaves C as it is
    for kern in ("auto", "mfma_64x64_dma5", "naive"):
        h.set_kernel(kern)
        c.fill_(float("nan"))
        h.sgemm_batched(0, 0, m, n, 0, a.data_ptr(), 1, 0, b.data_ptr(), n, 0, c.data_ptr(), ldc, sc, batch, True, s)
        torch.cuda.synchronize()
        assert bool(c.isnan().all())
        h.sgemm_batched(1, 1, m, n, 0, a.data_ptr(), m, 0, b.data_ptr(), 1, 0, c.data_ptr(), ldc, sc, batch, False, s)
        torch.cuda.synchronize()
        inside = torch.zeros(c.shape, dtype=torch.bool, device="cuda")
        for i in range(batch):
            inside[i * sc:i * sc + m * ldc].view(m, ldc)[:, :n] = True
        assert bool((c[inside] == 0).all()) and not bool(torch.signbit(c[inside]).any())
        assert bool(c[~inside].isnan().all())
    h.set_kernel("auto")
    # refusals: nothing launched, C untouched
    c.fill_(float("nan"))
    bad = [
        dict(sc=(m - 1) * ldc + n - 1, status=H.ERR_INVALID_ARG),   # C matrices overlap by one element
        dict(sc=0, status=H.ERR_INVALID_ARG),
        dict(sa=-1, status=H.ERR_INVALID_ARG),
        dict(batch=-1, status=H.ERR_INVALID_ARG),
        dict(ta=2, status=H.ERR_INVALID_ARG),
        dict(kernel="mfma", status=H.ERR_UNSUPPORTED),
        dict(kernel="mfma_96x96_dma5", status=H.ERR_UNSUPPORTED),
    ]
    for case in bad:
        h.set_kernel(case.get("kernel", "auto"))
        with pytest.raises(H.MMultError) as e:
            h.sgemm_batched(case.get("ta", 0), 0, m, n, k, a.data_ptr(), k, case.get("sa", m * k), b.data_ptr(), n, k * n,
                            c.data_ptr(), ldc, case.get("sc", sc), case.get("batch", batch), False, s)
        assert e.value.status == case["status"], case
    h.set_kernel("auto")
    torch.cuda.synchronize()
    assert bool(c.isnan().all())


def test_a_batch_beyond_the_workgroup_cap_goes_out_as_several_launches(h):
    import torch
    import how_to_optimize_gemm_amd as H
    batch = H.BATCHED_MAX_WORKGROUPS + 4097
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.rand(batch, device="cuda", generator=g) * 2 - 1
    b = torch.rand(batch, device="cuda", generator=g) * 2 - 1
    c = torch.full((batch,), float("nan"), device="cuda")
    h.set_kernel("auto")
    h.sgemm_batched(0, 0, 1, 1, 1, a.data_ptr(), 1, 1, b.data_ptr(), 1, 1, c.data_ptr(), 1, 1, batch, False,
                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    launch = H.last_launch()
    assert "sgemm_mfma_dma5_batched_kernel" in launch and "as 2 launches" in launch, launch
    want = (a.cpu().numpy() * b.cpu().numpy()).astype(np.float32)
    assert np.array_equal(c.cpu().numpy(), want)


def test_64_bit_matrix_offsets(h, oracle):
    import torch
    m = n = k = 64
    sa = (1 << 31) + 64
    big = torch.empty(sa + m * k, device="cuda")   # ~8.6 GB
    try:
        rng = np.random.default_rng(3)
        A = [rng.uniform(-1, 1, (m, k)).astype(np.float32) for _ in range(2)]
        Bm = rng.uniform(-1, 1, (2, k, n)).astype(np.float32)
        big[:m * k].copy_(torch.from_numpy(A[0].ravel()))
        big[sa:sa + m * k].copy_(torch.from_numpy(A[1].ravel()))
        b = torch.from_numpy(Bm.ravel()).cuda()
        s = torch.cuda.current_stream().cuda_stream
        for kern in ("auto", "mfma_64x64_dma5", "naive"):
            h.set_kernel(kern)
            c = torch.full((2 * m * n,), float("nan"), device="cuda")
            h.sgemm_batched(0, 0, m, n, k, big.data_ptr(), k, sa, b.data_ptr(), n, k * n, c.data_ptr(), n, m * n, 2, False, s)
            got = c.cpu().numpy().reshape(2, m, n)
            for i in range(2):
                assert same_bits(got[i], oracle.ref_mmult(A[i], Bm[i], fma=True)), (kern, i)
    finally:
        h.set_kernel("auto")
        del big
        torch.cuda.empty_cache()


@pytest.mark.parametrize("m,batch,marker", [(256, 64, "batch 64"), (2176, 2, "as a loop of 2")])
def test_a_captured_batched_launch_replays_the_eager_bits(h, m, batch, marker):
    import torch
    import how_to_optimize_gemm_amd as H
    h.set_kernel("auto")
    a = torch.rand((batch, m, m), device="cuda") - 0.5
    b = torch.rand((batch, m, m), device="cuda") - 0.5
    eager = h.bmm(a, b.transpose(1, 2))
    torch.cuda.synchronize()
    assert marker in H.last_launch(), H.last_launch()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    h.reserve_stream(side.cuda_stream, m, m, m)
    c = torch.full((batch, m, m), float("nan"), device="cuda")
    graph = torch.cuda.CUDAGraph()
    bt = b.transpose(1, 2)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            h.bmm(a, bt, out=c)
    for rep in range(2):
        c.fill_(float("nan"))
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(c, eager), rep


def test_bmm_takes_views_broadcasts_and_out(h, oracle):
    import torch
    import how_to_optimize_gemm_amd as H
    h.set_kernel("auto")
    g = torch.Generator(device="cuda").manual_seed(9)
    batch, m, n, k = 6, 70, 90, 45
    a = torch.rand((batch, m, k), device="cuda", generator=g) - 0.5
    b = torch.rand((batch, k, n), device="cuda", generator=g) - 0.5

    def want(x, y, c=None):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        return np.stack([oracle.ref_mmult(np.ascontiguousarray(x[i]), np.ascontiguousarray(y[i]),
                                          None if c is None else c[i].copy(), fma=True) for i in range(x.shape[0])])

    assert same_bits(h.bmm(a, b).cpu().numpy(), want(a, b))
    at = a.transpose(1, 2).contiguous().transpose(1, 2)   # (batch, m, k) with stride(1) == 1
    bt = b.transpose(1, 2).contiguous().transpose(1, 2)
    assert same_bits(h.bmm(at, bt).cpu().numpy(), want(a, b))
    a1 = a[:1].expand(batch, m, k)                        # batch stride 0
    b1 = b[:1].expand(batch, k, n)
    assert same_bits(h.bmm(a1, b).cpu().numpy(), want(a1, b))
    assert same_bits(h.bmm(a, b1).cpu().numpy(), want(a, b1))
    assert same_bits(h.bmm(at[:1].expand(batch, m, k), b1).cpu().numpy(), want(a1, b1))
    c0 = torch.rand((batch, m, n), device="cuda", generator=g)
    out = c0.clone()
    h.bmm(a, bt, out=out, accumulate=True)
    assert same_bits(out.cpu().numpy(), want(a, b, c0.cpu().numpy()))
    big = torch.full((batch, m + 3, n + 5), float("nan"), device="cuda")   # out as a strided window
    h.bmm(a, b, out=big[:, :m, :n])
    assert same_bits(big[:, :m, :n].cpu().numpy(), want(a, b))
    assert bool(big[:, m:, :].isnan().all()) and bool(big[:, :, n:].isnan().all())
    with pytest.raises(H.MMultError):
        h.bmm(a, b, out=torch.empty((1, m, n), device="cuda").expand(batch, m, n))   # every C matrix the same memory
    with pytest.raises(H.MMultError):
        h.bmm(a[0], b[0])
    assert h.bmm(a[:0], b[:0]).shape == (0, m, n)


def _best_ms(fns, bursts=5):
    for f in fns.values():
        f()
    ms = {name: [] for name in fns}
    for _ in range(bursts):
        for name, f in fns.items():
            ms[name].append(f())
    return {name: min(v) for name, v in ms.items()}


def test_batched_rate_floors(h):
    """AUTO on 256 x 256^3 at >= 3x a loop of 256 mmh_sgemm calls (each of those fills 16 of 256 CUs); AUTO on 64 x 1024^3
    at >= 0.85 of NN 4096^3, the same flop count.  Interleaved bursts in one process."""
    import torch
    h.set_kernel("auto")
    s = torch.cuda.current_stream().cuda_stream
    m, batch = 256, 256
    a = torch.rand((batch, m, m), device="cuda") - 0.5
    b = torch.rand((batch, m, m), device="cuda") - 0.5
    c = torch.empty((batch, m, m), device="cuda")
    sz = m * m

    def batched():
        return h.time_sgemm_batched(0, 0, m, m, m, a.data_ptr(), m, sz, b.data_ptr(), m, sz, c.data_ptr(), m, sz, batch, 1, 10, s)

    def loop():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 10
        e0.record()
        for _ in range(reps):
            for i in range(batch):
                h.sgemm(m, m, m, a.data_ptr() + 4 * i * sz, m, b.data_ptr() + 4 * i * sz, m, c.data_ptr() + 4 * i * sz, m, False, s)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    best = _best_ms({"batched": batched, "loop": loop})
    print(f"256 x 256^3: batched {best['batched']:.4f} ms, loop of 256 mmh_sgemm {best['loop']:.4f} ms, "
          f"{best['loop'] / best['batched']:.2f}x")
    assert best["loop"] / best["batched"] >= 3.0, best

    m, batch, N = 1024, 64, 4096
    a = torch.rand((batch, m, m), device="cuda") - 0.5
    b = torch.rand((batch, m, m), device="cuda") - 0.5
    c = torch.empty((batch, m, m), device="cuda")
    sz = m * m
    a4, b4, c4 = (torch.rand((N, N), device="cuda") - 0.5 for _ in range(3))
    best = _best_ms({
        "batched": lambda: h.time_sgemm_batched(0, 0, m, m, m, a.data_ptr(), m, sz, b.data_ptr(), m, sz, c.data_ptr(), m, sz, batch,
                                                1, 10, s),
        "nn4096": lambda: h.time_sgemm_op(0, 0, N, N, N, a4.data_ptr(), N, b4.data_ptr(), N, c4.data_ptr(), N, 1, 10, s),
    })
    print(f"64 x 1024^3: batched {best['batched']:.4f} ms, NN 4096^3 {best['nn4096']:.4f} ms, "
          f"{best['nn4096'] / best['batched']:.3f} of NN")
    assert best["nn4096"] / best["batched"] >= 0.85, best


def test_batched_fuzz_against_the_naive_batched_kernel():
    """tools/fuzz.py --batched: random shapes, strides, ops, bases and accumulate flags, AUTO and the three tiles forced,
    each bit-equal to sgemm_naive_batched_kernel, nothing written outside the C matrices."""
    import subprocess
    import sys
    from conftest import REPO
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "fuzz.py"), "--batched", "60", "0", "2031"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "fuzz --batched: 60 cases x 4 variants, 0 failures" in r.stdout, r.stdout[-500:]
