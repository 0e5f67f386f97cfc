"""GPU parity tests (run with -m gpu on an MI355X).  Everything goes through
the C ABI (libmmult_hip.so); the oracle is only the checker.

Bars:
  * bit-exact against the FUSED reference chain (the reference's
    REF_MMult as built with FMA contraction, i.e. aarch64/makefile:14):
    gfx950's f32 MFMA is an fmaf chain over ascending k, and so are K0/K1;
  * max-abs-diff against the UNFUSED reference chain (x86 -O2 build of
    armv7/REF_MMult.c) <= TOL(k) = 2e-7 * k + 1e-6 -- i.e. <= 8.2e-4 at
    k=4096, against the harness's own 0.5 (cuda/test_MMult.cpp:123-127) and
    the reference's published 3.5e-4 at 4096 (cuda/output_MMult_cuda_12.m:29);
  * integer-valued inputs: exactly equal (diff == 0), like every checked-in
    aarch64/armv7 output file.
"""
import numpy as np
import pytest

from gpu_operands import dev

from conftest import golden_cases, load_golden

pytestmark = pytest.mark.gpu

KERNELS = ["mfma", "mfma256", "mfma_256x256", "mfma_128x64", "mfma_64x64", "auto", "mfma_pipe", "mfma_simple", "valu",
           "valu_128x128", "valu_64x64", "naive", "mfma_64x64_dma", "mfma_128x64_dma", "mfma_128x128_dma",
    "mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5", "mfma_96x96_dma5"]


def tol(k):
    return 2e-7 * k + 1e-6


def run_strided(mm, a_buf, b_buf, c_buf, m, n, k, accumulate):
    """a_buf (m x lda), b_buf (k x ldb), c_buf (m x ldc) numpy; device pointers +
    leading dimensions go to mmh_sgemm untouched."""
    import torch
    da, db, dc = dev(a_buf), dev(b_buf), dev(c_buf)
    mm.sgemm(m, n, k, da.data_ptr(), a_buf.shape[1], db.data_ptr(), b_buf.shape[1],
             dc.data_ptr(), c_buf.shape[1], accumulate, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dc.cpu().numpy()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", golden_cases())
def test_golden_fixtures_device_flavour(mm, name, kernel):
    g = load_golden(name)
    mm.set_kernel(kernel)
    acc = name.startswith("accumulate")
    # poison C when overwriting: the device flavour never reads C (cuda/test_MMult.cpp:89)
    c_in = g["c0"].copy() if acc else np.full_like(g["c0"], np.nan)
    got = run_strided(mm, g["a"], g["b"], c_in, g["m"], g["n"], g["k"], acc)
    n = g["n"]
    assert np.array_equal(got[:, :n], g["c_ref_fma"][:, :n]), "not bit-equal to the fused reference chain"
    assert np.abs(got[:, :n] - g["c_ref"][:, :n]).max() <= tol(g["k"])
    if not acc:   # padding columns of C (ldc > n) must be left untouched
        assert np.isnan(got[:, n:]).all()


@pytest.mark.parametrize("name", golden_cases())
def test_golden_fixtures_host_flavour(mm, oracle, name):
    """MY_MMult(m,n,k,a,lda,b,ldb,c,ldc) on host buffers, C += A*B
    (armv7/test_MMult.c:71-76)."""
    g = load_golden(name)
    mm.set_kernel("mfma")
    c = g["c0"].copy()
    mm.MY_MMult(g["m"], g["n"], g["k"], g["a"], g["lda"], g["b"], g["ldb"], c, g["ldc"])
    n = g["n"]
    assert np.array_equal(c[:, :n], g["c_ref_fma"][:, :n])
    assert np.array_equal(c[:, n:], g["c0"][:, n:])
    d, _ = oracle.compare_matrices(c[:, :n], g["c_ref"][:, :n])
    assert d <= tol(g["k"])


@pytest.mark.parametrize("shape", [(64, 64, 64), (512, 512, 512), (300, 200, 100), (2048, 1024, 512)])
def test_vulkan_flavour_returns_the_chain_and_a_device_time(mm, oracle, shape):
    """`float MY_MMult(m, n, k, a, b, c)` (vulkan/test_MMult.cpp:10,55): dense row-major host buffers,
    C = A*B whatever C held, returns the GEMM's device milliseconds."""
    m, n, k = shape
    a, b = oracle.harness_inputs(m, n, k, seed=77 + m)
    c = np.full((m, n), np.nan, dtype=np.float32)
    mm.set_kernel("auto")
    ms = mm.MY_MMult_ms(m, n, k, a, b, c)
    assert np.array_equal(c, oracle.ref_mmult(a, b, fma=True))
    assert 0.0 < ms < 50.0


SHAPES = [(256, 256, 256), (384, 640, 1024), (128, 128, 32), (128, 256, 4096), (1000, 1000, 1000),
          (130, 129, 37), (3, 5, 7), (257, 255, 513), (512, 128, 2048), (1024, 1024, 1024)]


@pytest.mark.parametrize("kernel", ["mfma", "mfma256", "mfma_256x256", "mfma_128x64", "mfma_64x64", "valu", "valu_64x64"])
@pytest.mark.parametrize("shape", SHAPES)
def test_seeded_inputs_vs_oracle(mm, oracle, shape, kernel):
    m, n, k = shape
    a, b = oracle.harness_inputs(m, n, k, seed=1000 + m + n + k)
    mm.set_kernel(kernel)
    got = mm.matmul(dev(a), dev(b)).cpu().numpy()
    assert np.array_equal(got, oracle.ref_mmult(a, b, fma=True))
    assert oracle.compare_matrices(got, oracle.ref_mmult(a, b, fma=False))[0] <= tol(k)


@pytest.mark.parametrize("kernel", ["mfma_64x64_dma", "mfma_128x64_dma", "mfma_128x128_dma",
    "mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5", "mfma_96x96_dma5"])
def test_lds_dma_small_tile_kernel_is_the_same_chain(mm, oracle, kernel):
    """K2L (sgemm_dma.hpp): both operands by LDS-DMA into a ring of K-slice buffers, A as a ROW-major
    image read with ds_read2st64_b32.  Same MFMA, same k order -> the oracle's bits, for one slice, for
    slice counts on every phase of the ring (1 .. 7, 16, 18 slices of 64), overwrite and accumulate;
    ragged shapes run the GUARDED instantiation of the same tile (round 3), or -- with MMH_OPT_DMA_EDGE = 0 --
    fall back to the register-staged kernel as they did in round 2."""
    import torch
    import how_to_optimize_gemm_amd as H
    mm.set_kernel(kernel)
    bm, bn = (int(x) for x in kernel.split("_")[1].split("x"))
    for (m, n, k) in [(bm, bn, 64), (bm, bn, 128), (bm, 2 * bn, 192), (2 * bm, 3 * bn, 256), (256, 256, 320), (bm, 256, 384),
                      (bm, bn, 448), (1024, 1024, 1024), (1152 if bm <= 128 else 1280,) * 3, (256, 2048, 64), (bm, bn, 4096),
                      (bm, bn, 32 if bn == 128 else 64), (bm, bn, 96 if bn == 128 else 192)]:
        a, b = oracle.harness_inputs(m, n, k, seed=m + 3 * n + 5 * k)
        got = mm.matmul(dev(a), dev(b)).cpu().numpy()
        assert "LDS-DMA" in H.last_launch(), (m, n, k, H.last_launch())     # plain or stream-K launch of the DMA tile
        assert mm.streamk_timeouts() == 0
        want = oracle.ref_mmult(a, b, fma=True)
        assert np.array_equal(got, want), (kernel, m, n, k, float(np.abs(got - want).max()))
        c0 = np.random.default_rng(k).uniform(-1, 1, (m, n)).astype(np.float32)
        out = dev(c0)
        mm.matmul(dev(a), dev(b), out=out, accumulate=True)
        assert np.array_equal(out.cpu().numpy(), oracle.ref_mmult(a, b, c0.copy(), fma=True)), (kernel, m, n, k)
    # views with leading dimensions larger than the rows (multiples of 4 floats keep it on the DMA path)
    a, b = oracle.harness_inputs(256, 384, 128, seed=3)
    abuf = torch.zeros((256, 136), device="cuda")
    bbuf = torch.zeros((128, 388), device="cuda")
    cbuf = torch.full((256, 392), float("nan"), device="cuda")
    abuf[:, :128] = dev(a)
    bbuf[:, :384] = dev(b)
    mm.matmul(abuf[:, :128], bbuf[:, :384], out=cbuf[:, :384])
    assert "LDS-DMA" in H.last_launch()
    assert np.array_equal(cbuf[:, :384].cpu().numpy(), oracle.ref_mmult(a, b, fma=True))
    assert torch.isnan(cbuf[:, 384:]).all()
    for (m, n, k) in [(130, 129, 37), (256, 256, 100), (1000, 1000, 1000)]:     # ragged: the guarded DMA tile, same bits
        a, b = oracle.harness_inputs(m, n, k, seed=m)
        got = mm.matmul(dev(a), dev(b)).cpu().numpy()
        assert "LDS-DMA" in H.last_launch() and "guarded" in H.last_launch(), H.last_launch()
        assert np.array_equal(got, oracle.ref_mmult(a, b, fma=True))
        mm.set_option(H.OPT_DMA_EDGE, 0)                                         # ... or, switched off, the round-2 fall-back
        try:
            got = mm.matmul(dev(a), dev(b)).cpu().numpy()
            assert "LDS-DMA" not in H.last_launch()
            assert np.array_equal(got, oracle.ref_mmult(a, b, fma=True))
        finally:
            mm.set_option(H.OPT_DMA_EDGE, 2)
    # ragged tile counts: the same tile under the chained stream-K control flow, with and without
    if True:
        for (m, n, k) in [(1152, 1152, 512), (1536, 1536, 256), (1792, 1280, 192), (2176, 2176, 128), (2944, 2432, 64),
                          (4352, 4352, 64)]:
            if m % bm or n % bn:
                continue
            a, b = oracle.harness_inputs(m, n, k, seed=m + n)
            da, db = dev(a), dev(b)
            mm.set_streamk(True)
            got = mm.matmul(da, db)
            launched = H.last_launch()
            c0 = torch.rand((m, n), device="cuda")
            acc = c0.clone()
            mm.matmul(da, db, out=acc, accumulate=True)
            mm.set_streamk(False)
            plain = mm.matmul(da, db)
            assert "LDS-DMA" in H.last_launch() and "streamk" not in H.last_launch()
            mm.set_streamk(True)
            assert torch.equal(got, plain), (kernel, m, n, k, launched)
            assert mm.streamk_timeouts() == 0
            assert np.array_equal(got.cpu().numpy(), oracle.ref_mmult(a, b, fma=True))
            assert np.array_equal(acc.cpu().numpy(), oracle.ref_mmult(a, b, c0.cpu().numpy(), fma=True))



def test_headline_size_4096(mm, oracle):
    """BASELINE.json configs[2]: N=4096, MFMA kernel, the reference's input
    recipe (cuda/test_MMult.cpp:77-81) with a fixed seed."""
    n = 4096
    a, b = oracle.harness_inputs(n, n, n, seed=0x1234ABCD)
    mm.set_kernel("mfma")
    got = mm.matmul(dev(a), dev(b)).cpu().numpy()
    fused = oracle.ref_mmult(a, b, fma=True)
    assert np.array_equal(got, fused)
    unfused = oracle.ref_mmult(a, b, fma=False)
    d, _ = oracle.compare_matrices(got, unfused)
    assert d <= tol(n), d                    # <= 8.2e-4; the harness itself allows 0.5
    # the GPU's error against fp64 is no worse than the reference loop's own
    c64 = oracle.ref_mmult_f64(a, b)
    assert np.abs(got - c64).max() <= 1.05 * np.abs(unfused - c64).max() + 1e-6
    # every kernel variant is the same chain -> identical bits.  "auto" is what bench.py and the
    # harness run at this size: it launches the 128x64 K2W tile (LDS-DMA by loader waves) on a plain launch (2048
    # tiles = four whole rounds of two workgroups per CU; round 3 ran K2L's 128x64 tile here, round 2 the 256x256 tile),
    # and that launch -- like the K2L tiles and the 256x256 tile -- is checked here against the oracle on the FULL
    # matrix, not on sampled rows.
    import how_to_optimize_gemm_amd as H
    for kern in ("auto", "mfma_256x256", "mfma_64x64_dma", "mfma_128x64_dma", "mfma_128x64_dma5", "mfma_64x64_dma5", "mfma256",
                 "mfma_tiles", "mfma_128x64", "valu", "valu_128x128"):
        mm.set_kernel(kern)
        out = mm.matmul(dev(a), dev(b)).cpu().numpy()
        if kern == "mfma_256x256":
            assert "sgemm_mfma_kernel<256,256>" in H.last_launch(), (kern, H.last_launch())
        if kern == "mfma_64x64_dma":
            assert "sgemm_mfma_dma_kernel<64,64>" in H.last_launch() and "4096 workgroups" in H.last_launch(), (kern, H.last_launch())
        if kern == "mfma_128x64_dma":
            assert "sgemm_mfma_dma_kernel<128,64>" in H.last_launch() and "2048 workgroups" in H.last_launch(), (kern, H.last_launch())
        if kern in ("auto", "mfma_128x64_dma5"):
            assert "sgemm_mfma_dma5_kernel<128,64>" in H.last_launch() and "2048 workgroups" in H.last_launch(), (kern, H.last_launch())
        assert np.array_equal(out, fused), kern
    # accumulate mode at the headline size, through the headline kernel: C's value starts each chain
    mm.set_kernel("auto")
    c0 = np.random.default_rng(11).uniform(-1, 1, (n, n)).astype(np.float32)
    out = dev(c0)
    mm.matmul(dev(a), dev(b), out=out, accumulate=True)
    assert np.array_equal(out.cpu().numpy(), oracle.ref_mmult(a, b, c0.copy(), fma=True))


@pytest.mark.parametrize("shape,expect", [
    ((4352, 4352, 4352), "streamk_kernel<256,256>"),    # 289 tiles on 256 workgroups: unguarded stream-K
    ((5000, 5000, 256), "streamk_kernel<256,256>"),     # 400 ragged tiles: guarded stream-K
    ((4000, 4000, 520), "sgemm_mfma_kernel<256,256>"),  # 256 ragged tiles: guarded plain launch, ragged K
    ((4608, 4096, 1000), "streamk_kernel<256,256>"),    # 288 tiles, k not a multiple of the slice
])
def test_big_tile_full_matrix_vs_oracle(mm, oracle, shape, expect):
    """The 256x256 configuration in all four launch forms (plain / stream-K x unguarded / guarded) at
    sizes with at least one tile per CU, every element of C against the fused oracle chain."""
    import how_to_optimize_gemm_amd as H
    m, n, k = shape
    a, b = oracle.harness_inputs(m, n, k, seed=3 * m + 5 * n + 7 * k)
    mm.set_kernel("mfma_256x256")
    got = mm.matmul(dev(a), dev(b)).cpu().numpy()
    assert expect in H.last_launch(), H.last_launch()
    assert mm.streamk_timeouts() == 0
    assert np.array_equal(got, oracle.ref_mmult(a, b, fma=True))
    d, _ = oracle.compare_matrices(got, oracle.ref_mmult(a, b, fma=False))
    assert d <= tol(k)
    # whatever AUTO picks for the shape (4352^3 and the ragged counts of 256x256 tiles: the 128x64 LDS-DMA tile
    # as a phase-ordered stream-K launch, guarded where the shape is ragged; 4000 x 4000: the guarded 256x256
    # tile) -- the same bits
    mm.set_kernel("auto")
    assert np.array_equal(mm.matmul(dev(a), dev(b)).cpu().numpy(), got), H.last_launch()
    assert mm.streamk_timeouts() == 0
    if shape == (4352, 4352, 4352):
        assert "sgemm_dma5_streamk_kernel" in H.last_launch() and "chained parts" in H.last_launch(), H.last_launch()


def test_sweep_sizes_integer_pattern_exact(mm, oracle):
    """The reference sweep p = 1024..4096 step 128 (cuda/parameters.h:5-7),
    sampled, with the (j-i)%3 known-answer inputs: diff must be exactly 0."""
    import torch
    mm.set_kernel("mfma")
    for p in (1024, 1152, 2048, 2944, 4096):
        a, b = oracle.harness_inputs(p, p, p, pattern=3)
        got = mm.matmul(dev(a), dev(b))
        want = torch.from_numpy(a).cuda().double() @ torch.from_numpy(b).cuda().double()
        assert torch.equal(got.double(), want), p


def test_size_independent_properties_at_full_size(mm):
    """Exact algebraic properties of a k-ordered fmaf chain, N=4096."""
    import torch
    mm.set_kernel("mfma")
    g = torch.Generator(device="cuda").manual_seed(7)
    n = 4096
    a = torch.rand((n, n), device="cuda", generator=g) * 2 - 1
    b = torch.rand((n, n), device="cuda", generator=g) * 2 - 1
    c = mm.matmul(a, b)
    # determinism run-to-run
    assert torch.equal(c, mm.matmul(a, b))
    # row permutation of A permutes rows of C bit-for-bit
    perm = torch.randperm(n, device="cuda", generator=g)
    assert torch.equal(mm.matmul(a[perm].contiguous(), b), c[perm])
    # column permutation of B permutes columns of C bit-for-bit
    assert torch.equal(mm.matmul(a, b[:, perm].contiguous()), c[:, perm])
    # power-of-two scaling is exact
    assert torch.equal(mm.matmul(a * 4.0, b * 0.5), c * 2.0)
    # identity: A * I == A exactly
    eye = torch.eye(n, device="cuda")
    assert torch.equal(mm.matmul(a, eye), a)
    # a sub-problem (row panel x column panel) reproduces the same bits:
    # this is what the multi-GPU row-panel shard relies on
    sub = mm.matmul(a[1024:1536], b[:, 2048:2560].contiguous())
    assert torch.equal(sub, c[1024:1536, 2048:2560])
    # views with leading dimensions larger than the row length
    sub2 = mm.matmul(a[512:640, :], b[:, 128:384])        # ldb = 4096 > n = 256
    assert torch.equal(sub2, c[512:640, 128:384])


@pytest.mark.parametrize("kernel,sk,shape", [
    ("mfma_128x64_dma", 1, (2944, 2944, 2944)),     # 1058 tiles on 512 workgroups
    ("mfma_128x64_dma", 1, (4352, 4352, 256)),      # 2312 tiles on 512
    ("mfma_64x64_dma", 2, (2560, 2560, 512)),       # 1600 tiles on 768 (forced: the policy prefers the plain launch)
    ("mfma_128x128_dma", 1, (2944, 3072, 384)),     # 552 tiles on 256
    ("mfma", 1, (3968, 3968, 200)),                 # register-staged 128x128 tile (961 tiles on 512), ragged K
    ("mfma", 1, (4097, 4095, 70)),                  # guarded: ragged edges and K
    ("mfma_256x256", 1, (7000, 7000, 96)),          # 784 guarded 256x256 tiles on 256
])
def test_phase_ordered_stream_k_keeps_the_bits(mm, oracle, kernel, sk, shape):
    """MMH_OPT_STREAMK_ORDER (default on): from 1.8 tiles per workgroup a stream-K launch takes its ranges
    in K-phase order and its tiles in a matching placement (two per-shape tables) -- a different
    assignment of the same (tile, K-range) parts to workgroups, so C is the same chain: bit-equal to the
    launch with ranges in plain order, to one workgroup per tile, and to the oracle; overwrite and
    accumulate; repeated launches (the cached tables) as well."""
    import torch
    import how_to_optimize_gemm_amd as H
    m, n, k = shape
    a, b = oracle.harness_inputs(m, n, k, seed=m + 3 * n + 11 * k)
    da, db = dev(a), dev(b)
    mm.set_kernel(kernel)
    mm.set_streamk(sk)
    try:
        assert mm.get_option(H.OPT_STREAMK_ORDER) == 1
        got = mm.matmul(da, db)
        assert "streamk" in H.last_launch(), H.last_launch()
        again = mm.matmul(da, db)                       # second launch: tables from the cache
        mm.set_option(H.OPT_STREAMK_ORDER, 0)
        plain_order = mm.matmul(da, db)
        mm.set_option(H.OPT_STREAMK_ORDER, 1)
        assert mm.streamk_timeouts() == 0
        assert torch.equal(got, again) and torch.equal(got, plain_order)
        mm.set_kernel("mfma_tiles")
        assert torch.equal(got, mm.matmul(da, db))
        if m * n * k <= 3000 * 3000 * 3000:
            assert np.array_equal(got.cpu().numpy(), oracle.ref_mmult(a, b, fma=True))
        c0 = torch.rand((m, n), device="cuda")
        want = c0.clone()
        mm.matmul(da, db, out=want, accumulate=True)    # one workgroup per tile
        mm.set_kernel(kernel)
        out = c0.clone()
        mm.matmul(da, db, out=out, accumulate=True)
        assert "streamk" in H.last_launch()
        assert torch.equal(out, want)
    finally:
        mm.set_option(H.OPT_STREAMK_ORDER, 1)
        mm.set_streamk(True)


@pytest.mark.parametrize("shape", [(2176, 2176, 2176), (3072, 3072, 1024), (2560, 3200, 512),
                                   (2944, 2944, 2944), (3328, 2304, 96),
                                   # guarded stream-K: ragged edges, ragged K, odd leading dimensions
                                   (2049, 2049, 200), (2177, 2305, 333), (4097, 4095, 70)])
def test_stream_k_is_bit_identical(mm, oracle, shape):
    """Ragged tile counts run as ONE persistent chained stream-K launch: a tile
    split between two workgroups is still one fmaf chain over ascending k
    (the second workgroup continues from the first one's partial accumulators, handed over in
    a workspace slot), so the bits equal the one-workgroup-per-tile kernel's and the oracle's --
    for whole shapes and, through the guarded kernel, for any m, n, k and leading dimensions."""
    import torch
    m, n, k = shape
    a, b = oracle.harness_inputs(m, n, k, seed=m + 7 * n + 13 * k)
    da, db = dev(a), dev(b)
    mm.set_kernel("mfma")
    mm.set_streamk(True)
    got = mm.matmul(da, db)
    assert mm.streamk_timeouts() == 0
    import how_to_optimize_gemm_amd as H
    assert "streamk" in H.last_launch(), H.last_launch()      # the persistent launch really ran
    mm.set_kernel("mfma_tiles")
    ref = mm.matmul(da, db)
    assert torch.equal(got, ref)
    assert np.array_equal(got.cpu().numpy(), oracle.ref_mmult(a, b, fma=True))
    # accumulate mode: the head part starts from the caller's C, the tail from the partial
    c0 = torch.rand((m, n), device="cuda")
    c1, c2 = c0.clone(), c0.clone()
    mm.set_kernel("mfma")
    mm.matmul(da, db, out=c1, accumulate=True)
    mm.set_kernel("mfma_tiles")
    mm.matmul(da, db, out=c2, accumulate=True)
    assert torch.equal(c1, c2)
    # repeated launches reuse the flag buffer
    mm.set_kernel("mfma")
    for _ in range(5):
        mm.matmul(da, db, out=c1)
    assert torch.equal(c1, ref) and mm.streamk_timeouts() == 0
    # switch it off: same bits from the plain launch
    mm.set_streamk(False)
    assert torch.equal(mm.matmul(da, db), ref)
    mm.set_streamk(True)


def test_auto_on_large_ragged_shapes_uses_the_big_tile_and_keeps_the_bits(mm, oracle):
    """AUTO on large ragged shapes (whatever the cost table picks -- tests/test_auto_plan.py and
    test_the_host_plan_is_what_the_device_launches pin the choice; round 3's rules ran the guarded 256x256 tile at
    4000 x 4000 and the guarded 64x64 tile at 5000 x 5000): a guarded launch, the same bits as one workgroup per
    128x128 tile and as the oracle; and with K = 16384 (B beyond the Infinity Cache: rounds 2-3 fenced that off for the
    256x256 tile) whatever the table says, the bits of the 256x256 tile's launch."""
    import torch
    import how_to_optimize_gemm_amd as H
    for (m, n, k) in [(4000, 4000, 40), (5000, 5000, 72), (4000, 4000, 1000)]:
        a, b = oracle.harness_inputs(m, n, k, seed=m + k)
        da, db = dev(a), dev(b)
        mm.set_kernel("auto")
        got = mm.matmul(da, db)
        assert "guarded" in H.last_launch(), H.last_launch()
        assert mm.streamk_timeouts() == 0
        mm.set_kernel("mfma_tiles")
        assert torch.equal(got, mm.matmul(da, db))
        assert np.array_equal(got.cpu().numpy(), oracle.ref_mmult(a, b, fma=True))
    mm.set_kernel("auto")
    x = torch.rand((512, 16384), device="cuda")
    y = torch.rand((16384, 4096), device="cuda")
    got = mm.matmul(x, y)
    name, tiles, grid = H.auto_plan(512, 4096, 16384)
    assert f"<{name.split('_')[1].replace('x', ',')}>" in H.last_launch(), (name, H.last_launch())
    mm.set_kernel("mfma_256x256")
    assert torch.equal(got, mm.matmul(x, y))
    mm.set_kernel("auto")


@pytest.mark.parametrize("kernel", ["mfma", "mfma_256x256", "mfma_128x64", "mfma_64x64", "valu"])
def test_subnormals_and_nonfinite_values_follow_the_chain(mm, oracle, kernel):
    """Edge values the reference loop would produce on the CPU must come out of the
    GPU chain the same way: subnormal products and sums are not flushed (the f32 MFMA
    keeps them, cdna guide section 3), infinities propagate, inf - inf / 0 * inf give NaN
    in exactly the same elements."""
    import torch
    mm.set_kernel(kernel)
    m, n, k = 128, 192, 96
    a, b = oracle.harness_inputs(m, n, k, seed=99)
    # subnormal territory: |a*b| ~ 1e-42, sums stay subnormal
    a_s, b_s = (a * np.float32(1e-21)).astype(np.float32), (b * np.float32(1e-21)).astype(np.float32)
    got = mm.matmul(dev(a_s), dev(b_s)).cpu().numpy()
    want = oracle.ref_mmult(a_s, b_s, fma=True)
    assert np.array_equal(got, want)
    assert np.any((want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)), "test must reach subnormals"
    # huge values: overflow to +-inf happens at the same partial sum
    a_h, b_h = (a * np.float32(3e19)).astype(np.float32), (b * np.float32(3e19)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        want = oracle.ref_mmult(a_h, b_h, fma=True)
    got = mm.matmul(dev(a_h), dev(b_h)).cpu().numpy()
    assert np.isinf(want).any()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    # planted inf / nan in the operands
    a_p, b_p = a.copy(), b.copy()
    a_p[3, 5] = np.inf
    a_p[70, 10] = -np.inf
    b_p[5, 7] = 0.0          # inf * 0 -> nan at C[3, 7]
    b_p[20, 100] = np.nan
    with np.errstate(invalid="ignore"):
        want = oracle.ref_mmult(a_p, b_p, fma=True)
    got = mm.matmul(dev(a_p), dev(b_p)).cpu().numpy()
    assert np.isnan(want[3, 7]) and np.isnan(want[:, 100]).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])


def test_accumulate_and_overwrite_semantics(mm, oracle):
    import torch
    a, b = oracle.harness_inputs(256, 384, 128, seed=31)
    c0 = np.random.default_rng(3).uniform(-1, 1, (256, 384)).astype(np.float32)
    for kernel in KERNELS:
        mm.set_kernel(kernel)
        out = dev(c0)
        mm.matmul(dev(a), dev(b), out=out, accumulate=True)
        want = oracle.ref_mmult(a, b, c0.copy(), fma=True)       # C's value starts the chain
        assert np.array_equal(out.cpu().numpy(), want), kernel
        out2 = dev(c0)
        mm.matmul(dev(a), dev(b), out=out2)                       # overwrite ignores old C
        assert np.array_equal(out2.cpu().numpy(), oracle.ref_mmult(a, b, fma=True)), kernel


def test_empty_and_degenerate_shapes(mm):
    import torch
    for kernel in KERNELS:
        mm.set_kernel(kernel)
        a = torch.zeros((0, 8), device="cuda")
        b = torch.zeros((8, 5), device="cuda")
        assert mm.matmul(a, b).shape == (0, 5)
        # k == 0: C = 0 on overwrite, C unchanged on accumulate
        c = torch.full((6, 5), 3.0, device="cuda")
        mm.matmul(torch.zeros((6, 0), device="cuda"), torch.zeros((0, 5), device="cuda"), out=c)
        assert torch.equal(c, torch.zeros_like(c))
        c.fill_(3.0)
        mm.matmul(torch.zeros((6, 0), device="cuda"), torch.zeros((0, 5), device="cuda"), out=c,
                  accumulate=True)
        assert torch.equal(c, torch.full_like(c, 3.0))


def test_invalid_arguments_return_codes(mm):
    import ctypes
    import how_to_optimize_gemm_amd as H
    import torch
    L = H.lib()
    t = torch.zeros((16, 16), device="cuda")
    p = t.data_ptr()
    h = mm._h
    assert L.mmh_sgemm(h, -1, 4, 4, p, 4, p, 4, p, 4, 0, None) == H.ERR_INVALID_ARG
    assert L.mmh_sgemm(h, 4, 4, 8, p, 4, p, 4, p, 4, 0, None) == H.ERR_INVALID_ARG   # lda < k
    assert L.mmh_sgemm(h, 4, 8, 4, p, 4, p, 4, p, 8, 0, None) == H.ERR_INVALID_ARG   # ldb < n
    assert L.mmh_sgemm(h, 4, 8, 4, p, 4, p, 8, p, 4, 0, None) == H.ERR_INVALID_ARG   # ldc < n
    assert L.mmh_sgemm(h, 4, 4, 4, None, 4, p, 4, p, 4, 0, None) == H.ERR_INVALID_ARG
    assert L.mmh_set_kernel(h, 99) == H.ERR_INVALID_ARG
    # the scheduling A/B variants and the timing-only ablation builds (wrong results) are not part of
    # the product library: their ids and int8 modes are rejected
    assert L.mmh_is_ab_build() == 0
    for kid in list(range(16, 20)) + list(range(21, 25)) + list(range(32, 45)):
        assert L.mmh_set_kernel(h, kid) == H.ERR_INVALID_ARG, kid
        assert H.kernel_name(kid) is None
    for mode in (1, 3, 4, 10, 11, 12, 13, 14, -1):
        assert L.mmh_set_option(h, H.OPT_IGEMM_MODE, mode) == H.ERR_INVALID_ARG, mode
    assert L.mmh_set_option(h, H.OPT_SPLITK, 17) == H.ERR_INVALID_ARG
    assert L.mmh_set_option(h, H.OPT_HOST_PANELS, 99) == H.ERR_INVALID_ARG
    assert L.mmh_set_option(h, 1234, 0) == H.ERR_INVALID_ARG
    # the torch glue checks what the kernels take on trust (dtype, device, overlapping rows)
    f = torch.zeros((8, 8), device="cuda")
    with pytest.raises(H.MMultError):
        mm.matmul(f.half(), f.half())
    with pytest.raises(H.MMultError):
        mm.matmul(f, f, out=torch.zeros((8, 8), device="cuda", dtype=torch.float16))
    with pytest.raises(H.MMultError):
        mm.matmul(torch.zeros((1, 8), device="cuda").expand(8, 8), f)          # stride(0) == 0
    with pytest.raises(H.MMultError):
        mm.igemm_s8(f.to(torch.int8), f.to(torch.int8), out=torch.zeros((8, 8), device="cuda"))   # fp32 out
    with pytest.raises(H.MMultError):
        mm.qgemm(f.double(), f.double())
    with pytest.raises(H.MMultError):
        mm.quantize_sym_s8(f.to(torch.int32))
    with pytest.raises(H.MMultError):
        mm.matmul_rocblas(f.half(), f)
    with pytest.raises(H.MMultError):
        mm.sgemm_host(np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32), c=np.zeros((4, 4), np.float64))
    with pytest.raises(H.MMultError):
        mm.sgemm_host(np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32), c=np.zeros((3, 4), np.float32))
    with pytest.raises(H.MMultError):
        mm.matmul(torch.zeros((4, 4)), torch.zeros((4, 4)))      # CPU tensors: no fallback
    # a second handle on a non-existent device
    hh = ctypes.c_void_p()
    assert L.mmh_create(ctypes.byref(hh), 4096) == H.ERR_NO_DEVICE


def test_unaligned_pointers_take_the_guarded_path(mm, oracle):
    import torch
    mm.set_kernel("mfma")
    a, b = oracle.harness_inputs(128, 128, 64, seed=77)
    buf_a = torch.zeros(128 * 64 + 1, device="cuda")
    buf_a[1:] = torch.from_numpy(a).cuda().reshape(-1)
    a_off = buf_a[1:].view(128, 64)                               # 4-byte aligned only
    got = mm.matmul(a_off, dev(b)).cpu().numpy()
    assert np.array_equal(got, oracle.ref_mmult(a, b, fma=True))


@pytest.mark.parametrize("kernel", ["mfma", "mfma256", "mfma_256x256", "mfma_128x64", "mfma_64x64", "mfma_64x64_dma",
                                    "mfma_128x64_dma", "mfma_128x128_dma", "auto",
    "mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5", "mfma_96x96_dma5"])
def test_misaligned_operands_and_odd_leading_dimensions(mm, oracle, kernel):
    """Every operand only 4-byte aligned, odd lda/ldb/ldc, ragged m/n/k, with
    poison around the matrices: the descriptor-bounded path must neither read
    poison into the result nor write outside C's m x n window."""
    import torch
    mm.set_kernel(kernel)
    for (m, n, k, lda, ldb, ldc) in [(300, 259, 101, 103, 261, 263), (128, 128, 32, 33, 129, 131),
                                     (257, 130, 64, 67, 133, 130), (513, 384, 250, 250, 384, 384)]:
        a, b = oracle.harness_inputs(m, n, k, seed=m + n + k)
        c0 = np.random.default_rng(1).uniform(-1, 1, (m, n)).astype(np.float32)
        bufs = {}
        for name, mat, ld in (("a", a, lda), ("b", b, ldb), ("c", c0, ldc)):
            rows, cols = mat.shape
            flat = torch.full((rows * ld + 1 + 64,), float("nan"), device="cuda")
            view = flat[1:1 + rows * ld].view(rows, ld)          # base is 4-byte aligned only
            view[:, :cols] = torch.from_numpy(mat).cuda()
            bufs[name] = (flat, view)
        for accumulate in (False, True):
            bufs["c"][1][:, :n] = torch.from_numpy(c0).cuda()
            mm.sgemm(m, n, k, bufs["a"][1].data_ptr(), lda, bufs["b"][1].data_ptr(), ldb,
                     bufs["c"][1].data_ptr(), ldc, accumulate, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = bufs["c"][1][:, :n].cpu().numpy()
            want = oracle.ref_mmult(a, b, c0.copy() if accumulate else None, fma=True)
            assert np.array_equal(got, want), (m, n, k, accumulate)
            # nothing outside the window was touched
            assert torch.isnan(bufs["c"][1][:, n:]).all()
            assert torch.isnan(bufs["c"][0][0]) and torch.isnan(bufs["c"][0][1 + m * ldc:]).all()


@pytest.mark.parametrize("kernel", ["mfma", "mfma_64x64_dma", "mfma_128x64_dma", "mfma_128x128_dma", "auto",
    "mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5", "mfma_96x96_dma5"])
def test_nonfinite_padding_does_not_leak_through_the_k_tail(mm, oracle, kernel):
    """k not a multiple of the K-slice: the loads run into the next row / the
    padding, which here holds inf/nan (A's padding, B's padding and the rows of the buffer below B);
    masked lanes must not poison C.  The LDS-DMA tiles cannot mask on the way in: they zero the fragments."""
    import torch
    mm.set_kernel(kernel)
    for (m, n, k, lda, ldb) in [(256, 256, 100, 104, 260), (128, 192, 37, 37, 193), (300, 130, 33, 64, 131), (64, 64, 1, 8, 64)]:
        a, b = oracle.harness_inputs(m, n, k, seed=9 + k)
        abuf = torch.full((m + 2, lda), float("inf"), device="cuda")
        abuf[:m, :k] = torch.from_numpy(a).cuda()
        bbuf = torch.full((k + 40, ldb), float("nan"), device="cuda")
        bbuf[:k, :n] = torch.from_numpy(b).cuda()
        got = mm.matmul(abuf[:m, :k], bbuf[:k, :n]).cpu().numpy()
        assert np.array_equal(got, oracle.ref_mmult(a, b, fma=True)), (kernel, m, n, k)
    mm.set_kernel("mfma")


def test_huge_leading_dimension_uses_64bit_addressing(mm, oracle):
    """Offsets beyond the 2 GiB buffer-descriptor window must fall back to
    64-bit global addressing, not wrap.  (One tile, whole, B only: tests/test_gpu_reg_parity.py runs the 64-bit
    instantiations of every register-staged tile, whole and guarded, with A and with B beyond the window, and proves
    from window_ok which instantiation each shape reaches.)"""
    import torch
    mm.set_kernel("mfma")
    k, n, ldb = 544, 128, 1 << 20                     # (k-1)*ldb*4 B > 2 GiB
    a, b = oracle.harness_inputs(128, n, k, seed=5)
    big = torch.zeros((k, ldb), device="cuda")
    big[:, :n] = torch.from_numpy(b).cuda()
    got = mm.matmul(dev(a), big[:, :n]).cpu().numpy()
    assert np.array_equal(got, oracle.ref_mmult(a, b, fma=True))


def test_int8_bit_exact(mm, oracle):
    """BASELINE.json configs[4]: int8 in [-127,127], int32 accumulate; parity
    is unpinned in the reference (no int8 code in-tree) -- checked against the
    integer triple loop."""
    import torch
    rng = np.random.default_rng(2026)
    # (100, 90, 72): A dword-aligned but B not -> the packed-B path; (100, 90, 70): neither -> simple kernel
    for (m, n, k) in [(128, 128, 64), (256, 384, 512), (100, 92, 72), (129, 132, 136), (100, 90, 70), (100, 90, 72),
                      (300, 258, 264),
                      (129, 130, 131), (128, 128, 128), (384, 256, 1000), (200, 150, 90), (131, 258, 66),
                      (1024, 1024, 1024)]:
        a = rng.integers(-127, 128, (m, k), dtype=np.int8)
        b = rng.integers(-127, 128, (k, n), dtype=np.int8)
        got = mm.igemm_s8(dev(a), dev(b)).cpu().numpy()
        assert np.array_equal(got, oracle.ref_igemm_s8(a, b)), (m, n, k)
    # worst case magnitude: all +-127 at k = 4096 stays inside int32
    a = np.full((128, 4096), 127, dtype=np.int8)
    b = np.full((4096, 128), -127, dtype=np.int8)
    got = mm.igemm_s8(dev(a), dev(b))
    assert int(got.min()) == int(got.max()) == -127 * 127 * 4096
    # accumulate
    c0 = rng.integers(-1000, 1000, (256, 128), dtype=np.int32)
    a = rng.integers(-127, 128, (256, 192), dtype=np.int8)
    b = rng.integers(-127, 128, (192, 128), dtype=np.int8)
    out = dev(c0)
    mm.igemm_s8(dev(a), dev(b), out=out, accumulate=True)
    assert np.array_equal(out.cpu().numpy(), oracle.ref_igemm_s8(a, b, c0.copy()))


@pytest.mark.parametrize("mode", [2, 5, 6, 7, 8, 9])      # (1, 3, 4 -- K3 and the packed-B kernel: tools build, tests/test_tools_build.py)
def test_int8_every_kernel_bit_exact(mm, oracle, mode):
    """Each int8 kernel forced in turn (MMH_OPT_IGEMM_MODE: 2 simple, 5 / 6 B read in place by LDS-DMA with 128x128 /
    256x256 tiles, 8 / 9 the ping-pong
    schedule of the in-place 256x256 tile as a persistent launch / one workgroup per tile, 7 the same kernel on
    v_mfma_i32_16x16x32_i8 -- the instruction BASELINE.json configs[4] names) on whole, ragged and tiny shapes,
    odd and even slice counts (k around multiples of 128 and 256)."""
    rng = np.random.default_rng(900 + mode)
    mm.set_igemm_mode(mode)
    try:
        for (m, n, k) in [(256, 256, 128), (512, 768, 640), (100, 92, 72), (257, 255, 129), (300, 700, 1000),
                          (1, 1, 1), (3, 260, 5), (640, 128, 4096), (1280, 1024, 384), (256, 512, 127),
                          (256, 256, 257), (512, 256, 513), (130, 70, 255)]:
            a = rng.integers(-127, 128, (m, k), dtype=np.int8)
            b = rng.integers(-127, 128, (k, n), dtype=np.int8)
            got = mm.igemm_s8(dev(a), dev(b)).cpu().numpy()
            assert np.array_equal(got, oracle.ref_igemm_s8(a, b)), (mode, m, n, k)
        c0 = rng.integers(-1000, 1000, (300, 520), dtype=np.int32)
        a = rng.integers(-127, 128, (300, 200), dtype=np.int8)
        b = rng.integers(-127, 128, (200, 520), dtype=np.int8)
        out = dev(c0)
        mm.igemm_s8(dev(a), dev(b), out=out, accumulate=True)
        assert np.array_equal(out.cpu().numpy(), oracle.ref_igemm_s8(a, b, c0.copy())), mode
    finally:
        mm.set_igemm_mode(0)


def test_quantised_gemm_end_to_end(mm, oracle):
    """quantise -> int8 GEMM -> dequantise, against the CPU restatement of the
    same contract (parity unpinned: the reference has only prose for it)."""
    import torch
    rng = np.random.default_rng(77)
    # (4096, 4096, 192): the 256x256 kernel with the dequantisation in its epilogue; (333, 257, 129): scalar
    # tails of the quantisation passes and ragged tiles
    for (m, n, k) in [(128, 128, 128), (200, 150, 90), (512, 384, 1000), (333, 257, 129), (4096, 4096, 192)]:
        a = rng.uniform(-2, 2, (m, k)).astype(np.float32)
        b = rng.uniform(-0.5, 0.5, (k, n)).astype(np.float32)
        qa, sa = mm.quantize_sym_s8(dev(a))
        qa_ref, sa_ref = oracle.quantize_sym_s8(a)
        assert float(sa) == np.float32(sa_ref)
        assert np.array_equal(qa.cpu().numpy(), qa_ref)
        assert int(qa.min()) >= -127 and int(qa.abs().max()) == 127
        got = mm.qgemm(dev(a), dev(b)).cpu().numpy()
        qb_ref, sb_ref = oracle.quantize_sym_s8(b)
        acc = oracle.ref_igemm_s8(qa_ref, qb_ref)
        inv = np.float32(1.0) / (np.float32(sa_ref) * np.float32(sb_ref))
        want = acc.astype(np.float32) * inv
        assert np.array_equal(got, want), (m, n, k)
        # the two-pass form (int32 C, separate dequantisation; any forced int8 kernel) gives the same floats
        mm.set_igemm_mode(5)
        try:
            assert np.array_equal(mm.qgemm(dev(a), dev(b)).cpu().numpy(), want), (m, n, k)
        finally:
            mm.set_igemm_mode(0)
        # and it approximates the fp32 product to quantisation accuracy
        exact = a.astype(np.float64) @ b.astype(np.float64)
        assert np.abs(got - exact).max() <= 0.02 * np.abs(exact).max() + 0.05


def test_int8_headline_4096(mm, oracle):
    """BASELINE.json configs[4] at its own size: the FULL 4096 x 4096 int32 matrix of the shipped kernel against the
    int32 triple loop of the oracle (threaded; seconds), every forced kernel -- the config-named 16x16x32 instruction
    (mode 7) among them -- against the same integers."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randint(-127, 128, (4096, 4096), device="cuda", dtype=torch.int8, generator=g)
    b = torch.randint(-127, 128, (4096, 4096), device="cuda", dtype=torch.int8, generator=g)
    got = mm.igemm_s8(a, b)
    want = oracle.ref_igemm_s8(a.cpu().numpy(), b.cpu().numpy())
    assert np.array_equal(got.cpu().numpy(), want)
    try:
        for mode in (5, 6, 7, 8, 9):
            mm.set_igemm_mode(mode)
            assert torch.equal(mm.igemm_s8(a, b), got), mode
    finally:
        mm.set_igemm_mode(0)


def test_int8_persistent_tiles_bit_exact(mm, oracle):
    """K3p walks several 256x256 tiles per workgroup once there are more tiles than CUs: the next tile's prologue is
    requested in front of the finished tile's C stores and its first two waits count past them.  Whole and ragged
    tile grids of 2 .. 5 tiles per CU, short K (the stores of a tile are still in flight when the next one ends),
    accumulate, the dequantising epilogue, and the one-workgroup-per-tile launch of the same kernel (mode 9)."""
    import torch
    rng = np.random.default_rng(66)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    side = 256 * int(np.ceil(np.sqrt(2.2 * cus)))            # ~2.2 tiles per CU, whole tiles
    shapes = [(side, side, 128), (side, side, 256), (side, side + 256, 640), (side + 3, side - 5, 384),
              (256 * (cus + 1), 256, 128), (256, 256 * (4 * cus + 3), 256), (3 * side // 2, 2 * side, 1000)]
    for (m, n, k) in shapes:
        a = torch.from_numpy(rng.integers(-127, 128, (m, k), dtype=np.int8)).cuda()
        b = torch.from_numpy(rng.integers(-127, 128, (k, n), dtype=np.int8)).cuda()
        want = torch.from_numpy(oracle.ref_igemm_s8(a.cpu().numpy(), b.cpu().numpy())).cuda()
        for mode in (0, 8, 9, 7):
            mm.set_igemm_mode(mode)
            try:
                got = mm.igemm_s8(a, b)
                assert torch.equal(got, want), (mode, m, n, k)
                for rep in range(3):                          # back to back: nothing left behind in the ring
                    assert torch.equal(mm.igemm_s8(a, b, out=got), want), (mode, m, n, k, rep)
            finally:
                mm.set_igemm_mode(0)
        c0 = torch.from_numpy(rng.integers(-1000, 1000, (m, n), dtype=np.int32)).cuda()
        out = c0.clone()
        mm.igemm_s8(a, b, out=out, accumulate=True)
        assert torch.equal(out, want + c0), (m, n, k)
    # the dequantising epilogue over several tiles per workgroup
    m = n = side
    k = 192
    af = torch.from_numpy(rng.uniform(-2, 2, (m, k)).astype(np.float32)).cuda()
    bf = torch.from_numpy(rng.uniform(-0.5, 0.5, (k, n)).astype(np.float32)).cuda()
    got = mm.qgemm(af, bf).cpu().numpy()
    qa_ref, sa_ref = oracle.quantize_sym_s8(af.cpu().numpy())
    qb_ref, sb_ref = oracle.quantize_sym_s8(bf.cpu().numpy())
    inv = np.float32(1.0) / (np.float32(sa_ref) * np.float32(sb_ref))
    assert np.array_equal(got, oracle.ref_igemm_s8(qa_ref, qb_ref).astype(np.float32) * inv)


def test_rocblas_comparator_agrees(mm, oracle):
    import how_to_optimize_gemm_amd as H
    a, b = oracle.harness_inputs(512, 768, 1024, seed=9)
    try:
        ref = mm.matmul_rocblas(dev(a), dev(b)).cpu().numpy()
    except H.MMultError as e:
        if e.status == H.ERR_UNSUPPORTED:
            pytest.skip("rocBLAS not loadable")
        raise
    mm.set_kernel("mfma")
    got = mm.matmul(dev(a), dev(b)).cpu().numpy()
    assert np.abs(got - ref).max() <= 5e-4       # different summation order inside the vendor kernel


def test_single_process_shard_with_one_device(mm, oracle):
    import how_to_optimize_gemm_amd as H
    a, b = oracle.harness_inputs(300, 200, 96, seed=12)
    c, t = H.sgemm_sharded(1, a, b)
    assert np.array_equal(c, oracle.ref_mmult(a, b, fma=True))
    assert t["bcast"] >= 0 and t["gemm"] > 0


def test_shard_handle_is_persistent_and_refuses_missing_devices(mm, oracle):
    """mmh_shard_create/_sgemm/_destroy: one handle, many calls (communicator, streams, buffers and the
    per-device product handles persist; shapes may change from call to call), stream-K per device, and
    a request for more devices than are visible FAILS (MMH_ERR_NO_DEVICE) -- it never runs on fewer."""
    import torch
    import how_to_optimize_gemm_amd as H
    visible = torch.cuda.device_count()
    with pytest.raises(H.MMultError) as e:
        H.ShardedMMult(visible + 1)
    assert e.value.status == H.ERR_NO_DEVICE and "fewer visible devices" in str(e.value)
    with pytest.raises(H.MMultError):
        H.ShardedMMult(1, devices=[visible])                       # ordinal out of range
    for g in sorted({1, visible}):
        with H.ShardedMMult(g, kernel="auto") as sh:
            info = sh.info()
            assert info["ngpus"] == g and info["rccl_ranks"] == (g if g > 1 else 0)
            for (m, n, k) in [(300, 200, 96), (3072, 3072, 128), (1024, 512, 2048)]:
                a, b = oracle.harness_inputs(m, n, k, seed=m + g)
                c, t = sh.sgemm(a, b, gemm_reps=3)
                assert np.array_equal(c, oracle.ref_mmult(a, b, fma=True)), (g, m, n, k)
                assert t["gemm"] > 0 and t["h2d"] > 0 and t["d2h"] > 0
                assert (t["bcast"] > 0) == (g > 1)


def test_row_panel_shard_reassembles_full_product(mm, oracle):
    """What N ranks would each compute (their mmh_shard_rows panel, full B),
    run serially on one GPU, equals the unsharded product bit-for-bit."""
    import how_to_optimize_gemm_amd as H
    import torch
    n = 1024
    a, b = oracle.harness_inputs(n, n, n, seed=1)
    da, db = dev(a), dev(b)
    mm.set_kernel("mfma")
    full = mm.matmul(da, db)
    for nranks in (2, 8):
        out = torch.empty_like(full)
        for r in range(nranks):
            r0, rows = H.shard_rows(n, nranks, r)
            mm.matmul(da[r0:r0 + rows], db, out=out[r0:r0 + rows])
        assert torch.equal(out, full)


def test_config4_panel_at_full_size_sampled_rows(mm, oracle):
    """BASELINE configs[3] at its real size: one rank's share of the N=16384 problem
    (rows mmh_shard_rows(16384, 8, r) of A, all of B = 1 GiB).  The full oracle would take
    minutes, so a deterministic sample of rows (first, last, tile edges) is checked
    bit-exactly against the fused chain, plus the size-independent sub-problem property."""
    import torch
    import how_to_optimize_gemm_amd as H
    n = 16384
    r0, rows = H.shard_rows(n, 8, 3)
    assert (r0, rows) == (6144, 2048)
    g = torch.Generator(device="cuda").manual_seed(16384)
    a = torch.rand((rows, n), device="cuda", generator=g) * 2 - 1
    b = torch.rand((n, n), device="cuda", generator=g) * 2 - 1
    mm.set_kernel("auto")
    c = mm.matmul(a, b)
    sample = [0, 1, 127, 128, 1000, 2047]
    want = oracle.ref_mmult(a[sample].cpu().numpy(), b.cpu().numpy(), fma=True)
    assert np.array_equal(c[sample].cpu().numpy(), want)
    # a 128-row slab of the panel computed on its own gives the same bits
    assert torch.equal(mm.matmul(a[512:640], b), c[512:640])
    del a, b, c
    torch.cuda.empty_cache()


def test_differential_fuzz_and_stream_k_stress():
    """tools/fuzz.py: random shapes / leading dimensions / misaligned bases / accumulate flags,
    every kernel variant bit-equal to the naive kernel and nothing written outside C's window;
    then repeated stream-K launches on ragged tile counts against the plain launch."""
    import os
    import subprocess
    import sys
    from conftest import REPO
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "fuzz.py"), "80", "15", "2026"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import re
    assert re.search(r"fuzz: 80 cases x \d+ variants, 0 failures", r.stdout), r.stdout[-500:]
    assert "stream-K stress: 0 failures" in r.stdout


def test_int8_differential_fuzz():
    """tools/fuzz_i8.py: every int8 kernel mode against the correctness-first kernel (and that one
    against fp64) on random shapes, leading dimensions, byte-misaligned bases, accumulate flags;
    nothing written outside C's window."""
    import os
    import subprocess
    import sys
    from conftest import REPO
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "fuzz_i8.py"), "60", "2026"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "int8 fuzz: 60 cases x 6 modes, 0 failures" in r.stdout


def test_launches_capture_into_a_hip_graph(mm, oracle):
    """mmh_sgemm / mmh_igemm_s8 only enqueue work on the caller's stream (returns before
    completion, harness synchronises): after one eager warm-up call (workspaces allocated, LDS
    opt-in done) a sequence of them captures into a hipGraph and replays with the same bits."""
    import torch
    rng = np.random.default_rng(31)
    shapes = [(256, 384, 512), (1280, 1152, 640), (300, 200, 100)]     # plain, stream-K (ragged tiles), guarded
    ops = []
    for (m, n, k) in shapes:
        a, b = oracle.harness_inputs(m, n, k, seed=m + n + k)
        ops.append((dev(a), dev(b), torch.empty((m, n), device="cuda")))
    qa = dev(rng.integers(-127, 128, (256, 512), dtype=np.int8))
    qb = dev(rng.integers(-127, 128, (512, 384), dtype=np.int8))
    qc = torch.empty((256, 384), device="cuda", dtype=torch.int32)
    mm.set_kernel("auto")
    eager = []
    for (a, b, c) in ops:                 # warm-up = the eager reference
        mm.matmul(a, b, out=c)
        eager.append(c.clone())
    mm.igemm_s8(qa, qb, out=qc)
    q_eager = qc.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for (m, n, k) in shapes:              # the capture stream needs a stream-K workspace set of its own (never borrowed)
        mm.reserve_stream(side.cuda_stream, m, n, k)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for (a, b, c) in ops:
                mm.matmul(a, b, out=c)
            mm.igemm_s8(qa, qb, out=qc)
    torch.cuda.current_stream().wait_stream(side)
    for rep in range(3):
        for (_, _, c) in ops:
            c.fill_(float("nan"))
        qc.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for (_, _, c), want in zip(ops, eager):
            assert torch.equal(c, want), rep
        assert torch.equal(qc, q_eager), rep
    assert mm.streamk_timeouts() == 0


def test_peak_probes_are_sane(mm):
    tf = mm.probe_mfma_f32()
    assert 100.0 < tf < 165.0, tf          # 157.3 TFLOP/s is the fp32 MFMA peak
    gb = mm.probe_hbm_copy(1 << 30)
    assert 2000.0 < gb < 8000.0, gb


def test_split_k_timeout_is_a_sticky_error(oracle):
    """The only kernels that still WAIT for another workgroup are the opt-in split-K finishers (stream-K's
    hand-over is wait-free, see test_stream_k_needs_no_co_residency).  Fault injection: split-K producers do
    not announce their partial tiles, every finisher runs into the (shortened) spin limit, stops WITHOUT
    storing, and the handle turns sticky: the NEXT mmh_* call -- and every one after it -- fails with
    MMH_ERR_HIP, no polling needed.  Clearing the word makes the handle usable again, same bits."""
    import torch
    import how_to_optimize_gemm_amd as H
    h = H.MMult(0, "mfma_splitk")
    try:
        m = n = 1024                                   # 64 tiles of 128x128 for 256 CUs: split-K's case
        k = 2048
        a, b = oracle.harness_inputs(m, n, k, seed=5)
        da, db = dev(a), dev(b)
        h.set_splitk(4)
        good = h.matmul(da, db)
        assert "splitk" in H.last_launch(), H.last_launch()
        assert h.streamk_timeouts() == 0
        h.set_option(H.OPT_STREAMK_SPIN_LIMIT, 4)      # 4096 polls instead of seconds
        h.set_option(H.OPT_FAULT_INJECT, 1)
        h.matmul(da, db)                               # asynchronous: the launch itself is accepted
        torch.cuda.synchronize()
        with pytest.raises(H.MMultError) as e:         # ... and the next call on the handle reports it
            h.matmul(da, db)
        assert e.value.status == H.ERR_HIP and "timed out" in str(e.value)
        with pytest.raises(H.MMultError):              # sticky: still failing, whatever the entry point
            h.probe_mfma_f32()
        h.set_option(H.OPT_FAULT_INJECT, 0)
        with pytest.raises(H.MMultError):
            h.matmul(da, db)
        assert h.streamk_timeouts() > 0
        h.clear_error()
        h.set_option(H.OPT_STREAMK_SPIN_LIMIT, 65536)
        assert torch.equal(h.matmul(da, db), good) and h.streamk_timeouts() == 0
        # time_sgemm synchronises, so it reports a timeout of its OWN launches
        h.set_option(H.OPT_STREAMK_SPIN_LIMIT, 4)
        h.set_option(H.OPT_FAULT_INJECT, 1)
        c = torch.empty((m, n), device="cuda")
        with pytest.raises(H.MMultError):
            h.time_sgemm(m, n, k, da.data_ptr(), k, db.data_ptr(), n, c.data_ptr(), n, warmup=0, reps=1)
        # a stream-K launch has nothing to time out on: fault injection does not touch it
        h.clear_error()
        h.set_kernel("mfma")
        a2, b2 = oracle.harness_inputs(3072, 3072, 256, seed=6)
        got = h.matmul(dev(a2), dev(b2))
        assert "streamk" in H.last_launch()
        torch.cuda.synchronize()
        assert h.streamk_timeouts() == 0
        assert np.array_equal(got.cpu().numpy(), oracle.ref_mmult(a2, b2, fma=True))
    finally:
        h.close()


@pytest.mark.parametrize("shape", [(1024, 1024, 1024), (1152, 1152, 1152), (1536, 1536, 1536), (1792, 1792, 1792),
                                   (1024, 2048, 4096), (1280, 1024, 512)])
@pytest.mark.parametrize("kernel,parts", [("mfma_splitk", 0), ("mfma_splitk", 2), ("mfma_splitk", 4),
                                          ("mfma_splitk_128x64", 0), ("mfma_splitk_128x64", 2), ("auto", 1)])
def test_opt_in_split_k_meets_the_harness_tolerance(mm, oracle, shape, kernel, parts):
    """MMH_OPT_SPLITK / MMH_KERNEL_MFMA_SPLITK trade the one-chain-per-element bits for concurrency on
    shapes with fewer tiles than the chip has slots.  Its own bar: |diff| vs the UNFUSED REF_MMult
    <= tol(k) = 2e-7 k + 1e-6 (the harness's is 0.5, cuda/test_MMult.cpp:123-127), error vs fp64 no
    worse than 1.05x the reference loop's, deterministic run to run, exact on integer-valued inputs,
    and never used unless asked for."""
    import torch
    import how_to_optimize_gemm_amd as H
    m, n, k = shape
    a, b = oracle.harness_inputs(m, n, k, seed=m + n + k + parts)
    da, db = dev(a), dev(b)
    mm.set_kernel(kernel)
    mm.set_splitk(parts)
    try:
        got = mm.matmul(da, db)
        launched = H.last_launch()
        if "128x64" in kernel and "splitk" not in launched:
            # more 128x64 tiles x parts than workgroup slots: the launcher keeps the chain kernel
            assert np.array_equal(got.cpu().numpy(), oracle.ref_mmult(a, b, fma=True))
            return
        assert "splitk" in launched, launched
        assert mm.streamk_timeouts() == 0
        assert torch.equal(got, mm.matmul(da, db)), "split-K must be deterministic run to run"
        g = got.cpu().numpy()
        unfused = oracle.ref_mmult(a, b, fma=False)
        d, _ = oracle.compare_matrices(g, unfused)
        assert d <= tol(k), (d, launched)
        c64 = oracle.ref_mmult_f64(a, b)
        assert np.abs(g - c64).max() <= 1.05 * np.abs(unfused - c64).max() + 1e-6
        # accumulate: part 0 starts from C
        c0 = np.random.default_rng(2).uniform(-1, 1, (m, n)).astype(np.float32)
        out = dev(c0)
        mm.matmul(da, db, out=out, accumulate=True)
        d, _ = oracle.compare_matrices(out.cpu().numpy(), oracle.ref_mmult(a, b, c0.copy(), fma=False))
        assert d <= tol(k)
        # integer-valued inputs: every partial sum is exact, so the split changes nothing
        ai, bi = oracle.harness_inputs(m, n, k, pattern=3)
        want = torch.from_numpy(ai).cuda().double() @ torch.from_numpy(bi).cuda().double()
        assert torch.equal(mm.matmul(dev(ai), dev(bi)).double(), want)
    finally:
        mm.set_splitk(0)
    # default mode never splits: AUTO without the option is the chain, bit for bit
    mm.set_kernel("auto")
    assert np.array_equal(mm.matmul(da, db).cpu().numpy(), oracle.ref_mmult(a, b, fma=True))
    assert "splitk" not in H.last_launch()


def test_split_k_falls_back_to_the_chain_on_shapes_it_does_not_take(mm, oracle):
    import how_to_optimize_gemm_amd as H
    mm.set_splitk(4)
    try:
        for kernel in ("mfma_splitk", "mfma_splitk_128x64", "auto"):
            mm.set_kernel(kernel)
            for (m, n, k) in [(1000, 1000, 1000), (130, 129, 37), (1024, 1024, 32)]:   # ragged, or one K-slice
                a, b = oracle.harness_inputs(m, n, k, seed=m + k)
                got = mm.matmul(dev(a), dev(b)).cpu().numpy()
                assert "splitk" not in H.last_launch(), (kernel, m, n, k, H.last_launch())
                assert np.array_equal(got, oracle.ref_mmult(a, b, fma=True))
    finally:
        mm.set_splitk(0)
        mm.set_kernel("mfma")


@pytest.mark.parametrize("panels", [-1, 0, 2, 5, 16])
def test_host_flavour_pipeline_keeps_the_bits(oracle, panels):
    """mmh_sgemm_host's row-panel pipeline (copy-in / GEMM / copy-out on three streams) against the
    plain staged form and the oracle: C += A*B on host buffers with padded leading dimensions."""
    import how_to_optimize_gemm_amd as H
    h = H.MMult(0, "auto")
    try:
        h.set_host_panels(panels)
        for (m, n, k, lda, ldb, ldc) in [(2048, 1024, 512, 520, 1032, 1024), (1100, 640, 300, 300, 640, 648)]:
            rng = np.random.default_rng(m + panels)
            a = rng.uniform(-1, 1, (m, lda)).astype(np.float32)
            b = rng.uniform(-1, 1, (k, ldb)).astype(np.float32)
            c0 = rng.uniform(-1, 1, (m, ldc)).astype(np.float32)
            c = c0.copy()
            h.MY_MMult(m, n, k, a, lda, b, ldb, c, ldc)
            want = oracle.ref_mmult(a[:, :k], b[:, :n], c0.copy()[:, :n], fma=True)
            assert np.array_equal(c[:, :n], want), (panels, m)
            assert np.array_equal(c[:, n:], c0[:, n:])           # padding columns untouched
            for _ in range(2):                                    # the events are reused call after call
                c = c0.copy()
                h.MY_MMult(m, n, k, a, lda, b, ldb, c, ldc)
                assert np.array_equal(c[:, :n], want)
            # overwrite form
            got = h.sgemm_host(np.ascontiguousarray(a[:, :k]), np.ascontiguousarray(b[:, :n]))
            assert np.array_equal(got, oracle.ref_mmult(a[:, :k], b[:, :n], fma=True))
    finally:
        h.close()


def test_lds_probe_reads_a_plausible_rate(mm):
    """256 B/clk/CU x 256 CUs x 2.4 GHz = 157 TB/s is the LDS roof of the 8- and 16-byte reads
    (MI355X_MICROARCH.md, LDS), half that for ds_read_b32: the 16-byte fragment read must land within
    (50 %, 105 %) of it and the 4-byte read under 105 % of its own."""
    import how_to_optimize_gemm_amd as H
    wide = mm.probe_lds_read(16)
    assert 0.5 * 157300 < wide < 1.05 * 157300, wide
    assert 0 < mm.probe_lds_read(4) < 1.05 * 78600
    for w in (8, -8):
        assert 0 < mm.probe_lds_read(w) < 1.05 * 157300
    with pytest.raises(H.MMultError):
        mm.probe_lds_read(12)


def test_entry_points_restore_the_callers_device(mm):
    """Every entry point runs on the handle's device and leaves the thread's current device alone
    (with one visible GPU: the current device is 0 before and after, and a handle for another
    ordinal cannot be created)."""
    import torch
    before = torch.cuda.current_device()
    a = torch.rand((256, 256), device="cuda")
    mm.set_kernel("auto")
    mm.matmul(a, a)
    mm.probe_hbm_read(1 << 26)
    mm.sgemm_host(np.ones((64, 64), np.float32), np.ones((64, 64), np.float32))
    assert torch.cuda.current_device() == before
    if torch.cuda.device_count() > 1:
        import how_to_optimize_gemm_amd as H
        with H.MMult(1, "mfma") as h1:
            b = torch.rand((256, 256), device="cuda:1")
            torch.cuda.set_device(0)
            out = h1.matmul(b, b)
            assert torch.cuda.current_device() == 0 and out.device.index == 1
            with pytest.raises(H.MMultError):
                h1.matmul(a, a)                                   # tensors of another device


def test_quantiser_handles_tiny_and_non_finite_inputs(mm, oracle):
    """The contract's edge cases (quant_s8.hpp): the scale is taken over the FINITE elements, is
    clamped when 127 / max|x| would overflow, NaN quantises to 0 and +-inf to +-127."""
    import torch
    rng = np.random.default_rng(8)
    x = rng.uniform(-1, 1, (64, 96)).astype(np.float32)
    for case in ("tiny", "subnormal", "nonfinite", "zeros"):
        y = x.copy()
        if case == "tiny":
            y *= np.float32(1e-38)
        elif case == "subnormal":
            y = (y * np.float32(1e-30)).astype(np.float32) * np.float32(1e-12)
        elif case == "nonfinite":
            y[0, 0], y[1, 1], y[2, 2] = np.nan, np.inf, -np.inf
        else:
            y[:] = 0
        q, s = mm.quantize_sym_s8(dev(y))
        want_q, want_s = oracle.quantize_sym_s8(y)
        assert np.array_equal(q.cpu().numpy(), want_q), case
        assert float(s.item()) == want_s and np.isfinite(want_s) and want_s > 0, (case, want_s)
        if case == "nonfinite":
            assert want_q[0, 0] == 0 and want_q[1, 1] == 127 and want_q[2, 2] == -127
            assert np.abs(want_q).max() == 127 and (np.abs(want_q) == 127).sum() >= 3
