"""The int8 side's test vocabulary: a Case (shape, leading dimensions, base offsets), the launchers' host arithmetic restated
(`reach`: which instantiation a call launches and what mmh_last_launch then says), guarded device buffers, the exact integer
reference, and the functions that run one mmh_igemm_s8 / mmh_quantize_sym_s8 / mmh_qgemm_f32 call and compare it.  Serves
tests/test_gpu_int8_parity.py (whose table INSTANTIATIONS is made of these cases), tests/test_int8_coverage.py and
tests/test_gpu_int8_graph.py.  (Shared test code: see tests/bitcmp.py.)"""
import dataclasses
import math
from typing import Optional

import numpy as np

NXCD = 8                       # XCDs: a persistent K3p grid is a multiple of it
GUARD_I32 = -2139062144        # 0x80808080: never a sum here
GUARD_I8 = 77
GUARD_F32 = -7777.25
INT32_MAX = (1 << 31) - 1


def _b(x):
    return "true" if x else "false"


# ---- the launchers' host arithmetic (igemm.hip, igemm_s8.hpp, igemm_s8_pp.hpp, quant_s8.hpp) ---------------------------
def inplace_ok(lda, oa, ldb, ob, k):
    """i8_dword and i8_window: dword-aligned operands whose byte offsets stay inside the descriptors' 2 GiB window."""
    lim = (1 << 31) - 4096
    return lda % 4 == 0 and oa % 4 == 0 and ldb % 4 == 0 and ob % 4 == 0 and 256 * lda + k < lim and \
        (k + 256) * ldb + 256 < lim


def big_tile(m, n, cus):
    """i8_big_tile: rounds of 256x256 tiles (one per CU) against rounds of 128x128 ones (two per CU)."""
    t256 = math.ceil(m / 256) * math.ceil(n / 256)
    t128 = math.ceil(m / 128) * math.ceil(n / 128)
    return math.ceil(t256 / cus) <= 0.6 * math.ceil(t128 / (2 * cus)) + 1e-9


def c_fast(m, n, ldc, oc_bytes, tile):
    """The whole-tile (EDGE = false) instantiation: whole tiles, ldc % 4 == 0 and a 16-byte aligned C."""
    return m % tile == 0 and n % tile == 0 and ldc % 4 == 0 and oc_bytes % 16 == 0


def quant_vec_ok(ld, off_bytes):
    """quant_vec_ok for X (the q images of the entry points are 4-byte aligned; ldq decides for quantize_kernel)."""
    return off_bytes % 16 == 0 and ld % 4 == 0


def pp_grid(m, n, cap):
    tiles = math.ceil(m / 256) * math.ceil(n / 256)
    grid = tiles
    if 0 < cap < grid:
        grid = cap // NXCD * NXCD if cap >= NXCD else cap
    return tiles, grid


def pp_grid_cap(mode, k, cus, env_cap):
    if mode == 9:
        return 0
    if env_cap > 0:
        return env_cap
    if mode == 8:
        return cus
    return cus if k <= 5120 else 0


def _pp(edge, deq, mfma_k, m, n, cap):
    tiles, grid = pp_grid(m, n, cap)
    form = f"persistent: {grid} workgroups walk {tiles} tiles" if grid < tiles else f"{tiles} workgroups, one per tile"
    return [f"igemm_s8_pp_kernel<{_b(edge)},{_b(deq)},{mfma_k}>"], [form]


def _launch_igemm_s8(mode, m, n, k, lda, oa, ldb, ob, ldc, oc_bytes, cus):
    if mode in (0, 5, 6) and inplace_ok(lda, oa, ldb, ob, k):
        big = mode == 6 or (mode == 0 and big_tile(m, n, cus))
        t, tm = (256, 8) if big else (128, 4)
        return [f"igemm_s8_dma_kernel<{t},{t},{tm},{_b(not c_fast(m, n, ldc, oc_bytes, t))},0,true>"]
    fast = m % 128 == 0 and n % 128 == 0 and k % 64 == 0 and lda % 16 == 0 and ldb % 4 == 0 and ldc % 4 == 0 and \
        oa % 16 == 0 and ob % 4 == 0 and oc_bytes % 16 == 0
    return [f"igemm_s8_simple_kernel<{_b(not fast)}>"]


@dataclasses.dataclass(frozen=True)
class Case:
    """m x n x k with leading dimensions (0: dense) and base offsets in elements (int8 for igemm's A / B, int32 for its
    C, float for qgemm's and the quantiser's tensors).  The quantiser takes X = m x n with ld = lda, offset oa."""
    m: int
    n: int
    k: int = 0
    lda: int = 0
    ldb: int = 0
    ldc: int = 0
    oa: int = 0
    ob: int = 0
    oc: int = 0
    mode: Optional[int] = None      # overrides the row's MMH_OPT_IGEMM_MODE
    entry: Optional[str] = None     # overrides the row's entry point
    values: str = "random"          # "random", "ties" (quantiser: exact .5 ties and -0.0)

    def lds(self, entry):
        """The leading dimensions as MMult._tensor_args passes them: a one-row window's is its column count."""
        if entry == "quantize":
            return (self.lda or self.n) if self.m > 1 else self.n, 0, 0
        lda = (self.lda or self.k) if self.m > 1 else self.k
        ldb = (self.ldb or self.n) if self.k > 1 else self.n
        ldc = (self.ldc or self.n) if self.m > 1 else self.n
        return lda, ldb, ldc


def reach(entry, mode, c, cus, env_cap=0):
    """(symbols the call launches, further words of mmh_last_launch) -- the launchers' choice restated."""
    lda, ldb, ldc = c.lds(entry)
    m, n, k = c.m, c.n, c.k
    if entry == "quantize":
        vi = quant_vec_ok(lda, 4 * c.oa)
        vo = vi and n % 4 == 0                     # q: a fresh tensor, ldq = cols
        return ["absmax_kernel", "quantize_kernel"], [f"absmax_kernel ({'vector' if vi else 'row'} path)",
                                                      f"quantize_kernel ({'vector' if vo else 'row'} path)"]
    if entry == "qgemm":
        ka, nb = (k + 15) & ~15, (n + 3) & ~3
        syms = ["absmax_kernel", "quantize_kernel"]
        words = [f"A on the {'vector' if quant_vec_ok(lda, 4 * c.oa) else 'row'} path",
                 f"B on the {'vector' if quant_vec_ok(ldb, 4 * c.ob) else 'row'} path"]
        if mode == 0 and inplace_ok(ka, 0, nb, 0, k):
            if big_tile(m, n, cus):
                s, w = _pp(not c_fast(m, n, ldc, 4 * c.oc, 256), True, 64, m, n, pp_grid_cap(0, k, cus, env_cap))
                syms, words = syms + s, words + w
            else:
                syms.append(f"igemm_s8_dma_kernel<128,128,4,{_b(not c_fast(m, n, ldc, 4 * c.oc, 128))},0,true>")
            return syms, words + ["dequantised in the epilogue"]
        return syms + _launch_igemm_s8(mode, m, n, k, ka, 0, nb, 0, nb, 0, cus) + ["dequantize_kernel"], words
    assert entry == "igemm", entry
    oc = 4 * c.oc
    if inplace_ok(lda, c.oa, ldb, c.ob, k) and (mode in (7, 8, 9) or (mode == 0 and big_tile(m, n, cus))):
        cap = pp_grid_cap(0 if mode == 7 else mode, k, cus, env_cap)
        return _pp(not c_fast(m, n, ldc, oc, 256), False, 32 if mode == 7 else 64, m, n, cap)
    if mode == 0 and not inplace_ok(lda, c.oa, ldb, c.ob, k):
        a_ok, b_ok = lda % 4 == 0 and c.oa % 4 == 0, ldb % 4 == 0 and c.ob % 4 == 0
        ka, nb = (lda if a_ok else (k + 15) & ~15), (ldb if b_ok else (n + 15) & ~15)
        if inplace_ok(ka, c.oa if a_ok else 0, nb, c.ob if b_ok else 0, k):
            words = ([] if a_ok else ["A copied to workspace"]) + ([] if b_ok else ["B copied to workspace"])
            return _launch_igemm_s8(0, m, n, k, ka, c.oa if a_ok else 0, nb, c.ob if b_ok else 0, ldc, oc, cus), words
    return _launch_igemm_s8(mode, m, n, k, lda, c.oa, ldb, c.ob, ldc, oc, cus), []


def _big_side(cus):
    """The smallest multiple of 256 whose square the default rule gives to the 256x256 tile."""
    s = 256
    while not big_tile(s, s, cus):
        s += 256
    return s


# ---- running a case -----------------------------------------------------------------------------------------------------
def _window(flat, rows, cols, ld, off):
    import torch
    return torch.as_strided(flat, (rows, cols), (ld, 1), off)


def _buffer(rows, cols, ld, off, dtype, guard):
    import torch
    flat = torch.full((off + max(rows - 1, 0) * ld + cols + 64,), guard, dtype=dtype, device="cuda")
    return flat, _window(flat, rows, cols, ld, off)


def reference(a, b, c0=None):
    """Exact: float64 partial sums of int8 products are integers below 2^53."""
    ref = (a.astype(np.float64) @ b.astype(np.float64)).astype(np.int64)
    if c0 is not None:
        ref += c0.astype(np.int64)
    assert np.abs(ref).max(initial=0) <= INT32_MAX, "the reference does not fit in int32: the case is out of contract"
    return ref


def _int8(rng, shape):
    x = rng.integers(-128, 128, shape, dtype=np.int8)
    if x.size:
        x.reshape(-1)[rng.integers(0, x.size, max(1, x.size // 64))] = -128   # -128 is in range, and often
    return x


def _check_c(flat, view, want, guard, what):
    import torch
    got = view.cpu().numpy()
    assert np.array_equal(got.astype(np.int64) if got.dtype == np.int32 else got, want), \
        f"{what}: {int((got != want).sum())} of {got.size} differ, first at {np.argwhere(got != want)[0].tolist()}"
    mask = torch.ones_like(flat, dtype=torch.bool)
    _window(mask, *view.shape, view.stride(0), view.storage_offset()).fill_(False)
    assert bool((flat[mask] == guard).all()), f"{what}: a value outside C's window changed"


def run_igemm(mm, inst_mode, c, rng, cus, accumulate, env_cap=0, words=()):
    import torch
    import how_to_optimize_gemm_amd as H
    mode = inst_mode if c.mode is None else c.mode
    lda, ldb, ldc = c.lds("igemm")
    a, b = _int8(rng, (c.m, c.k)), _int8(rng, (c.k, c.n))
    _, av = _buffer(c.m, c.k, lda, c.oa, torch.int8, GUARD_I8)
    _, bv = _buffer(c.k, c.n, ldb, c.ob, torch.int8, -GUARD_I8)
    av.copy_(torch.from_numpy(a))
    bv.copy_(torch.from_numpy(b))
    cflat, cv = _buffer(c.m, c.n, ldc, c.oc, torch.int32, GUARD_I32)
    c0 = rng.integers(-(1 << 20), 1 << 20, (c.m, c.n), dtype=np.int32) if accumulate else None
    if accumulate:
        cv.copy_(torch.from_numpy(c0))
    mm.set_igemm_mode(mode)
    try:
        mm.igemm_s8(av, bv, out=cv, accumulate=accumulate)
        torch.cuda.synchronize()
        launched = H.last_launch()
    finally:
        mm.set_igemm_mode(0)
    syms, more = reach("igemm", mode, c, cus, env_cap)
    what = f"mode {mode} {c} {'accumulate' if accumulate else 'overwrite'}: {launched}"
    for w in list(syms) + list(more) + list(words):
        assert w in launched, f"{what}: '{w}' not in the launch marker"
    _check_c(cflat, cv, reference(a, b, c0), GUARD_I32, what)
    return syms


def _quant_input(rng, rows, cols, values):
    if values == "ties":
        # max|x| = 127: scale 1 exactly, so every x.5 is a tie after scaling; -0.0 and both signs of the maximum
        x = (rng.integers(-254, 255, (rows, cols)) / 2.0).astype(np.float32)
        x.reshape(-1)[0] = -0.0
        x.reshape(-1)[-1] = 127.0
        if x.size > 2:
            x.reshape(-1)[x.size // 2] = -127.0
        return x
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    amax = np.float32(rng.uniform(0.5, 9.0))
    x = np.clip(x, -amax, amax)
    flat = x.reshape(-1)
    flat[rng.integers(0, flat.size)] = amax                  # late in the tensor: the largest workgroup index wins
    if flat.size > 1:
        flat[rng.integers(0, flat.size)] = -amax
    return x


def run_quantize(mm, c, rng):
    import torch
    import how_to_optimize_gemm_amd as H
    from oracle import oracle as O
    ld, _, _ = c.lds("quantize")
    x = _quant_input(rng, c.m, c.n, c.values)
    _, xv = _buffer(c.m, c.n, ld, c.oa, torch.float32, 1e30)   # a finite guard larger than every value: never read
    xv.copy_(torch.from_numpy(x))
    q, s = mm.quantize_sym_s8(xv)
    torch.cuda.synchronize()
    launched = H.last_launch()
    syms, words = reach("quantize", 0, c, 256)
    what = f"quantize {c}: {launched}"
    for w in syms + words:
        assert w in launched, f"{what}: '{w}' not in the launch marker"
    q_ref, s_ref = O.quantize_sym_s8(x)
    assert np.float32(s.item()).view(np.uint32) == np.float32(s_ref).view(np.uint32), (what, s.item(), s_ref)
    got = q.cpu().numpy()
    assert np.array_equal(got, q_ref), f"{what}: {int((got != q_ref).sum())} of {got.size} q differ"
    return syms


def run_qgemm(mm, inst_mode, c, rng, cus, env_cap=0, words=()):
    import torch
    import how_to_optimize_gemm_amd as H
    from oracle import oracle as O
    mode = inst_mode if c.mode is None else c.mode
    lda, ldb, ldc = c.lds("qgemm")
    a = rng.uniform(-2, 2, (c.m, c.k)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, (c.k, c.n)).astype(np.float32)
    _, av = _buffer(c.m, c.k, lda, c.oa, torch.float32, 1e30)
    _, bv = _buffer(c.k, c.n, ldb, c.ob, torch.float32, -1e30)
    av.copy_(torch.from_numpy(a))
    bv.copy_(torch.from_numpy(b))
    cflat, cv = _buffer(c.m, c.n, ldc, c.oc, torch.float32, GUARD_F32)
    mm.set_igemm_mode(mode)
    try:
        mm.qgemm(av, bv, out=cv)
        torch.cuda.synchronize()
        launched = H.last_launch()
    finally:
        mm.set_igemm_mode(0)
    syms, more = reach("qgemm", mode, c, cus, env_cap)
    what = f"qgemm mode {mode} {c}: {launched}"
    for w in syms + more + list(words):
        assert w in launched, f"{what}: '{w}' not in the launch marker"
    qa, sa = O.quantize_sym_s8(a)
    qb, sb = O.quantize_sym_s8(b)
    inv = np.float32(1.0) / (np.float32(sa) * np.float32(sb))
    want = reference(qa, qb).astype(np.float32) * inv
    _check_c(cflat, cv, want, GUARD_F32, what)
    return syms


def run_case(mm, inst, c, rng, cus, env_cap=0, words=()):
    entry = c.entry or inst.entry
    if entry == "quantize":
        return run_quantize(mm, c, rng)
    if entry == "qgemm":
        return run_qgemm(mm, inst.mode, c, rng, cus, env_cap, words)
    out = run_igemm(mm, inst.mode, c, rng, cus, False, env_cap, words)
    run_igemm(mm, inst.mode, c, rng, cus, True, env_cap, words)
    return out


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_igemm_view(mm, mode, av, b, syms):
    import torch
    import how_to_optimize_gemm_amd as H
    mm.set_igemm_mode(mode)
    try:
        out = mm.igemm_s8(av, torch.from_numpy(b).cuda())
        torch.cuda.synchronize()
        for s in syms:
            assert s in H.last_launch(), (s, H.last_launch())
        return out.cpu().numpy()
    finally:
        mm.set_igemm_mode(0)
