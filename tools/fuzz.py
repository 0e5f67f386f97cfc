#!/usr/bin/env python3
"""Differential fuzz on one GPU: every kernel variant against the naive kernel (an
independent code path with the same chain semantics -> bit-equal, signed zeros included:
same_bits) on random shapes, leading dimensions, 4-byte-misaligned bases and accumulate
flags; plus a stream-K stress loop (ragged tile counts, repeated launches; whole rounds
of the persistent grid) against the one-tile-per-workgroup kernel.
usage: python tools/fuzz.py [--ops | --batched | --ex] [cases] [stress_reps] [seed]
--ops: the transposed-operand forms instead (mmh_sgemm_op: NT / TN / TT on AUTO and the 64x64 / 128x64 / 128x128 LDS-DMA
tiles, plain and stream-K) against the naive kernel's op form, with NaN in every operand's padding and behind its last row.
--batched: mmh_sgemm_batched on random shapes, batch strides (gaps, strides that are not a multiple of 4, 0 = broadcast),
ops, bases and accumulate flags -- AUTO (fold, one launch or loop) and the three tiles forced -- against the naive batched
kernel, with NaN in every padding and gap, none of which may be written.
--ex: mmh_sgemm_ex (C = act(alpha op(A) op(B) + beta C + bias)) on random shapes, op pairs (NN included), leading dimensions,
misaligned bases and bias pointers and random epilogues -- AUTO and the three tiles, plain and stream-K -- against the naive
kernel's epilogue form, with NaN in every padding (and in C itself when beta == 0)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import how_to_optimize_gemm_amd as H  # noqa: E402

OPS = "--ops" in sys.argv
BATCHED = "--batched" in sys.argv
EX = "--ex" in sys.argv
argv = [x for x in sys.argv if x not in ("--ops", "--batched", "--ex")]
cases = int(argv[1]) if len(argv) > 1 else 200
stress = int(argv[2]) if len(argv) > 2 else 30
seed = int(argv[3]) if len(argv) > 3 else 1
rng = np.random.default_rng(seed)
mm = H.MMult(0)
stream = torch.cuda.current_stream().cuda_stream
VARIANTS = ["auto", "mfma", "mfma256", "mfma_256x256", "mfma_128x64", "mfma_64x64", "mfma_pipe", "mfma_simple", "valu",
            "valu_64x64", "valu_128x128", "mfma_64x64_dma", "mfma_128x64_dma", "mfma_128x128_dma",
            "mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5", "mfma_96x96_dma5",          # K2W (round 4)
            "mfma_64x64_dma5/sk2", "mfma_128x64_dma5/sk2", "mfma_128x128_dma5/sk2",                 # ... stream-K whenever ragged
            "mfma_96x64_dma5", "valu_128x64",                                                     # round 5: the 96x64 K2W tile, K1W's third tile
            "mfma_64x64_dma/sk2", "mfma_128x64_dma/sk2",                                          # ... K2L under stream-K (AUTO's candidates now)
            "valu_64x64/sk2", "valu_128x64/sk2", "valu_128x128/sk2",                             # round 6: K1W under K2W's stream-K body
            "mfma_160x160_dma5",                                                                  # round 6: the 160x160 K2W tile (every K2W tile: fragment reads spread)
            "mfma_64x64_dma5/sk2u", "mfma_128x128_dma5/sk2u",                                     # K2W stream-K, parts unchained (MMH_OPT_STREAMK_CHAIN = 0)
            "mfma_128x64_dma5/persist", "mfma_64x64_dma/persist"]                                 # whole rounds persistent too (MMH_OPT_PERSIST = 1)
# variant suffix -> (MMH_OPT_STREAMK, MMH_OPT_STREAMK_CHAIN, MMH_OPT_PERSIST)
FORMS = {"": (1, 1, 0), "sk2": (2, 1, 0), "sk0": (0, 1, 0), "sk2u": (2, 0, 0), "persist": (1, 1, 1)}


def set_form(kern):
    streamk, chain, persist = FORMS[kern.partition("/")[2]]
    mm.set_kernel(kern.split("/")[0])
    mm.set_streamk(streamk)
    mm.set_option(H.OPT_STREAMK_CHAIN, chain)
    mm.set_option(H.OPT_PERSIST, persist)


def same_bits(x, y):
    """Bit patterns equal wherever y is not NaN (-0.0 is not +0.0), NaN in the same places (payloads not compared)."""
    nx, ny = torch.isnan(x), torch.isnan(y)
    return torch.equal(nx, ny) and torch.equal(x.view(torch.int32).masked_fill(nx, 0), y.view(torch.int32).masked_fill(ny, 0))


def strided(rows, cols, ld, off, fill=None):
    flat = torch.full((rows * ld + off + 8,), float("nan"), device="cuda")
    view = flat[off:off + rows * ld].view(rows, ld)
    if fill is not None:
        view[:, :cols] = fill
    return flat, view


def random_shape():
    kind = rng.integers(0, 7)
    if kind == 4:      # whole tiles, 16-byte aligned bases and leading dimensions: what the LDS-DMA tiles take
        m, n = (int(rng.integers(1, 12)) * 128 for _ in range(2))
        k = int(rng.integers(1, 24)) * 64
    elif kind == 0:    # tile multiples
        m, n, k = (int(rng.integers(1, 9)) * 128 for _ in range(3))
    elif kind == 1:    # ragged small
        m, n, k = (int(rng.integers(1, 400)) for _ in range(3))
    elif kind == 2:    # ragged around tile edges
        m, n, k = (int(rng.integers(1, 6)) * 128 + int(rng.integers(-3, 4)) for _ in range(3))
    elif kind == 5:    # a few rows / columns past a 64-boundary: the K2W kernels' thin edge tiles
        m, n = (int(rng.integers(1, 20)) * 64 + int(rng.integers(0, 18)) for _ in range(2))
        k = int(rng.integers(1, 900))
    elif kind == 6:    # enough tiles for multi-part stream-K ranges, ragged
        m, n = (int(rng.integers(1100, 2600)) for _ in range(2))
        k = int(rng.integers(33, 700))
    else:              # thin
        m, n, k = int(rng.integers(1, 40)), int(rng.integers(1, 2000)), int(rng.integers(1, 1500))
    return kind, m, n, k


def fuzz_ops():
    """C = op(A) op(B) on the op forms' kernels against sgemm_naive_op_kernel (mmh_sgemm_op with MMH_KERNEL_NAIVE)."""
    variants = ["auto", "mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5",
                "mfma_64x64_dma5/sk2", "mfma_128x64_dma5/sk2", "mfma_128x128_dma5/sk2", "mfma_128x128_dma5/sk0"]
    nbad = 0
    for case in range(cases):
        kind, m, n, k = random_shape()
        ta, tb = [(0, 1), (1, 0), (1, 1)][int(rng.integers(0, 3))]
        ra, ca = (k, m) if ta else (m, k)   # A as stored
        rb, cb = (n, k) if tb else (k, n)
        pad = (lambda: 4 * int(rng.integers(0, 3))) if kind == 4 else (lambda: int(rng.integers(0, 9)))
        lda, ldb, ldc = ca + pad(), cb + pad(), n + pad()
        offs = [4 * int(rng.integers(0, 2)) if kind == 4 else int(rng.integers(0, 4)) for _ in range(3)]
        acc = bool(rng.integers(0, 2))
        _, av = strided(ra, ca, lda, offs[0], torch.rand((ra, ca), device="cuda") * 2 - 1)
        _, bv = strided(rb, cb, ldb, offs[1], torch.rand((rb, cb), device="cuda") * 2 - 1)
        c0 = torch.rand((m, n), device="cuda")
        results = {}
        for kern in ["naive"] + variants:
            set_form(kern)
            cflat, cv = strided(m, n, ldc, offs[2], c0)
            mm.sgemm_op(ta, tb, m, n, k, av.data_ptr(), lda, bv.data_ptr(), ldb, cv.data_ptr(), ldc, acc, stream)
            torch.cuda.synchronize()
            results[kern] = cv[:, :n].clone()
            if not (bool(torch.isnan(cv[:, n:]).all()) and bool(torch.isnan(cflat[:offs[2]]).all())):
                nbad += 1
                print(f"ops case {case} {kern}: wrote outside C window  m,n,k={m},{n},{k} op={ta}{tb}")
        for kern in variants:
            if not same_bits(results[kern], results["naive"]):
                nbad += 1
                d = (results[kern] - results["naive"]).abs().max().item()
                print(f"ops case {case} {kern}: != naive (max diff {d})  m,n,k={m},{n},{k} op={'NT'[ta]}{'NT'[tb]} "
                      f"ld={lda},{ldb},{ldc} off={offs} acc={acc}")
    set_form("mfma")
    print(f"fuzz --ops: {cases} cases x {len(variants)} variants, {nbad} failures")
    return nbad


def fuzz_ex():
    """The fused epilogue on the `ex` kernels against sgemm_naive_ex_kernel (mmh_sgemm_ex with MMH_KERNEL_NAIVE)."""
    variants = ["auto", "mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5",
                "mfma_64x64_dma5/sk2", "mfma_128x64_dma5/sk2", "mfma_128x128_dma5/sk2", "mfma_128x128_dma5/sk0"]
    nbad = 0
    for case in range(cases):
        kind, m, n, k = random_shape()
        ta, tb = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        ra, ca = (k, m) if ta else (m, k)   # A as stored
        rb, cb = (n, k) if tb else (k, n)
        pad = (lambda: 4 * int(rng.integers(0, 3))) if kind == 4 else (lambda: int(rng.integers(0, 9)))
        lda, ldb, ldc = ca + pad(), cb + pad(), n + pad()
        offs = [4 * int(rng.integers(0, 2)) if kind == 4 else int(rng.integers(0, 4)) for _ in range(3)]
        alpha = float(rng.choice([1.0, 0.0, -1.0, 0.7, -1.3, 3.0]))
        beta = float(rng.choice([0.0, 0.0, 1.0, 0.5, -2.0]))
        mode, act = int(rng.integers(0, 3)), int(rng.integers(0, 2))
        boff = int(rng.integers(0, 4))
        nb = n if mode == H.BIAS_COL else m
        bias = (torch.rand((nb + boff,), device="cuda") * 2 - 1)[boff:]
        _, av = strided(ra, ca, lda, offs[0], torch.rand((ra, ca), device="cuda") * 2 - 1)
        _, bv = strided(rb, cb, ldb, offs[1], torch.rand((rb, cb), device="cuda") * 2 - 1)
        c0 = torch.rand((m, n), device="cuda") * 2 - 1 if beta != 0.0 else None   # beta == 0: C is NaN all over
        results = {}
        for kern in ["naive"] + variants:
            set_form(kern)
            cflat, cv = strided(m, n, ldc, offs[2], c0)
            mm.sgemm_ex(ta, tb, m, n, k, alpha, av.data_ptr(), lda, bv.data_ptr(), ldb, beta, cv.data_ptr(), ldc,
                        bias.data_ptr() if mode else 0, mode, act, stream)
            torch.cuda.synchronize()
            results[kern] = cv[:, :n].clone()
            if not (bool(torch.isnan(cv[:, n:]).all()) and bool(torch.isnan(cflat[:offs[2]]).all()) and
                    bool(torch.isnan(cflat[offs[2] + m * ldc:]).all())):
                nbad += 1
                print(f"ex case {case} {kern}: wrote outside C window  m,n,k={m},{n},{k} op={ta}{tb}")
        if bool(torch.isnan(results["naive"]).any()):
            nbad += 1
            print(f"ex case {case} naive: NaN in the result  m,n,k={m},{n},{k}")
        for kern in variants:
            if not same_bits(results[kern], results["naive"]):
                nbad += 1
                d = (results[kern] - results["naive"]).abs().max().item()
                print(f"ex case {case} {kern}: != naive (max diff {d})  m,n,k={m},{n},{k} op={'NT'[ta]}{'NT'[tb]} "
                      f"ld={lda},{ldb},{ldc} off={offs} alpha={alpha} beta={beta} bias={mode}+{boff} act={act}")
    set_form("mfma")
    print(f"fuzz --ex: {cases} cases x {len(variants)} variants, {nbad} failures")
    return nbad


def fuzz_batched():
    """C_i = op(A_i) op(B_i) (+ C_i) through mmh_sgemm_batched against sgemm_naive_batched_kernel (MMH_KERNEL_NAIVE)."""
    variants = ["auto", "mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5"]
    nbad = 0
    forms = {}
    for case in range(cases):
        shape = int(rng.integers(0, 4))
        if shape == 0:     # many small matrices
            m, n, k = (int(rng.integers(1, 140)) for _ in range(3))
            batch = int(rng.integers(1, 300))
        elif shape == 1:   # whole tiles: the whole-tile form where the strides allow it
            m, n = (int(rng.integers(1, 5)) * 128 for _ in range(2))
            k = int(rng.integers(1, 12)) * 32
            batch = int(rng.integers(1, 40))
        elif shape == 2:   # around the tile edges (thin last rows / columns), K tails
            m, n = (int(rng.integers(1, 5)) * 64 + int(rng.integers(-2, 18)) for _ in range(2))
            k = int(rng.integers(1, 300))
            batch = int(rng.integers(1, 24))
        else:              # a few mid-size matrices
            m, n, k = (int(rng.integers(300, 1300)) for _ in range(3))
            batch = int(rng.integers(1, 5))
        ta, tb = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        ra, ca = (k, m) if ta else (m, k)
        rb, cb = (n, k) if tb else (k, n)
        whole = shape == 1 and bool(rng.integers(0, 2))
        pad = (lambda: 4 * int(rng.integers(0, 2))) if whole else (lambda: int(rng.integers(0, 5)))
        lda, ldb, ldc = ca + pad(), cb + pad(), n + pad()
        def stride(rows, ld, may_broadcast):
            if may_broadcast and rng.integers(0, 5) == 0:
                return 0
            return rows * ld + (4 * int(rng.integers(0, 3)) if whole else int(rng.integers(0, 7)))
        fold = not ta and rng.integers(0, 4) == 0   # packed A and C, shared B: AUTO folds
        sa = ra * lda if fold else stride(ra, lda, True)
        sb = 0 if fold else stride(rb, ldb, True)
        sc = m * ldc if fold else stride(m, ldc, False)
        offs = [4 * int(rng.integers(0, 2)) if whole else int(rng.integers(0, 4)) for _ in range(3)]
        acc = bool(rng.integers(0, 2))
        size = lambda rows, cols, ld, s, off: off + (batch - 1) * s + (rows - 1) * ld + cols + 8
        a = torch.full((size(ra, ca, lda, sa, offs[0]),), float("nan"), device="cuda")
        b = torch.full((size(rb, cb, ldb, sb, offs[1]),), float("nan"), device="cuda")
        c0 = torch.full((size(m, n, ldc, sc, offs[2]),), float("nan"), device="cuda")
        inside = torch.zeros(c0.shape, dtype=torch.bool, device="cuda")
        for i in range(batch):
            for flat, rows, cols, ld, s, off in ((a, ra, ca, lda, sa, offs[0]), (b, rb, cb, ldb, sb, offs[1])):
                if s or i == 0:
                    flat[off + i * s:off + i * s + rows * ld].view(rows, ld)[:, :cols] = torch.rand((rows, cols), device="cuda") * 2 - 1
            w = c0[offs[2] + i * sc:offs[2] + i * sc + m * ldc].view(m, ldc)[:, :n]
            w.copy_(torch.rand((m, n), device="cuda"))
            inside[offs[2] + i * sc:offs[2] + i * sc + m * ldc].view(m, ldc)[:, :n] = True
        results = {}
        for kern in ["naive"] + variants:
            mm.set_kernel(kern)
            c = c0.clone()
            mm.sgemm_batched(ta, tb, m, n, k, a.data_ptr() + 4 * offs[0], lda, sa, b.data_ptr() + 4 * offs[1], ldb, sb,
                             c.data_ptr() + 4 * offs[2], ldc, sc, batch, acc, stream)
            torch.cuda.synchronize()
            if kern == "auto":
                form = "folded" if "folded" in H.last_launch() else "loop" if "loop of" in H.last_launch() else "one launch"
                forms[form] = forms.get(form, 0) + 1
            results[kern] = c
            if not same_bits(c[~inside], c0[~inside]):
                nbad += 1
                print(f"batched case {case} {kern}: wrote outside the C matrices  m,n,k={m},{n},{k} batch={batch}")
        for kern in variants:
            if not same_bits(results[kern][inside], results["naive"][inside]):
                nbad += 1
                print(f"batched case {case} {kern}: != naive  m,n,k={m},{n},{k} batch={batch} op={'NT'[ta]}{'NT'[tb]} "
                      f"ld={lda},{ldb},{ldc} strides={sa},{sb},{sc} off={offs} acc={acc}: {H.last_launch()}")
    mm.set_kernel("auto")
    print(f"fuzz --batched: AUTO forms {forms}")
    print(f"fuzz --batched: {cases} cases x {len(variants)} variants, {nbad} failures")
    return nbad


if OPS:
    sys.exit(1 if fuzz_ops() else 0)
if BATCHED:
    sys.exit(1 if fuzz_batched() else 0)
if EX:
    sys.exit(1 if fuzz_ex() else 0)

bad = 0
for case in range(cases):
    kind, m, n, k = random_shape()
    aligned = kind == 4
    lda, ldb, ldc = k + int(rng.integers(0, 9)), n + int(rng.integers(0, 9)), n + int(rng.integers(0, 9))
    offs = [int(rng.integers(0, 4)) for _ in range(3)]
    if aligned:
        lda, ldb, ldc = k + 4 * int(rng.integers(0, 3)), n + 4 * int(rng.integers(0, 3)), n + 4 * int(rng.integers(0, 3))
        offs = [4 * int(rng.integers(0, 2)) for _ in range(3)]
    acc = bool(rng.integers(0, 2))
    a = torch.rand((m, k), device="cuda") * 2 - 1
    b = torch.rand((k, n), device="cuda") * 2 - 1
    c0 = torch.rand((m, n), device="cuda")
    _, av = strided(m, k, lda, offs[0], a)
    _, bv = strided(k, n, ldb, offs[1], b)
    results = {}
    for kern in ["naive"] + VARIANTS:
        set_form(kern)
        cflat, cv = strided(m, n, ldc, offs[2], c0)
        mm.sgemm(m, n, k, av.data_ptr(), lda, bv.data_ptr(), ldb, cv.data_ptr(), ldc, acc, stream)
        torch.cuda.synchronize()
        results[kern] = cv[:, :n].clone()
        pad_ok = bool(torch.isnan(cv[:, n:]).all()) and bool(torch.isnan(cflat[:offs[2]]).all())
        if not pad_ok:
            bad += 1
            print(f"case {case} {kern}: wrote outside C window  m,n,k={m},{n},{k} ld={lda},{ldb},{ldc}")
    for kern in VARIANTS:
        if not same_bits(results[kern], results["naive"]):
            bad += 1
            d = (results[kern] - results["naive"]).abs().max().item()
            print(f"case {case} {kern}: != naive (max diff {d})  m,n,k={m},{n},{k} ld={lda},{ldb},{ldc} "
                  f"off={offs} acc={acc}")
set_form("mfma")
print(f"fuzz: {cases} cases x {len(VARIANTS)} variants, {bad} failures")

# stream-K stress
sk_bad = 0


def stress_against(a, b, ref, kerns, n, want_word=None):
    global sk_bad
    for kern in kerns:
        set_form(kern)
        c = torch.empty_like(ref)
        for rep in range(stress):
            c.fill_(float("nan"))
            mm.matmul(a, b, out=c)
            if want_word and want_word not in H.last_launch():
                sk_bad += 1
                print(f"stream-K {kern} N={n}: not a {want_word} launch: {H.last_launch()}")
                break
            if not same_bits(c, ref):
                sk_bad += 1
                print(f"stream-K {kern} N={n} rep {rep}: mismatch, max diff {(c - ref).abs().max().item()}")
        if mm.streamk_timeouts():
            sk_bad += 1
            print(f"stream-K {kern} N={n}: hand-off timeouts reported")


for n in (1152, 1536, 1792, 2176, 2432, 2944, 3072, 3456, 3712, 4352, 4608, 2049, 2305, 3001):   # the last three: guarded stream-K
    a = torch.rand((n, n), device="cuda") * 2 - 1
    b = torch.rand((n, n), device="cuda") * 2 - 1
    mm.set_kernel("mfma_tiles")
    ref = mm.matmul(a, b)
    # "auto": the LDS-DMA tiles under stream-K below 4096, the 256x256 tile above; "mfma": the register-staged 128x128 tile
    stress_against(a, b, ref, ("auto", "mfma", "mfma_128x128_dma5/sk2", "mfma_64x64_dma5/sk2", "mfma_128x128_dma5/sk2u",
                               "valu_128x128/sk2", "valu_64x64/sk2", "valu"), n)
# whole rounds of the persistent grid (MMH_OPT_PERSIST): 6 tiles per CU, a whole number of rounds on 1, 2 or 3 per CU
cus = mm.device_info()["cu_count"]
for kern, bm, bn in (("mfma_128x128_dma5/persist", 128, 128), ("mfma_64x64_dma5/persist", 64, 64), ("mfma_128x64_dma/persist", 128, 64)):
    a = torch.rand((6 * bm, 96), device="cuda") * 2 - 1
    b = torch.rand((96, cus * bn), device="cuda") * 2 - 1
    set_form("mfma_tiles")
    ref = mm.matmul(a, b)
    stress_against(a, b, ref, (kern,), f"{6 * bm}x{cus * bn}x96", "persistent")
set_form("mfma")
print(f"stream-K stress: {sk_bad} failures")
sys.exit(1 if bad or sk_bad else 0)
