"""Device operands and handles of the GPU tests: NaN-padded buffers, the calls that run one GEMM on them and say whether
anything outside C's window was written, the shared inputs and oracle results of a shape, and the module-scoped fixtures
(handles, `cus`, `big`) that test modules import by name.  (Shared test code: see tests/bitcmp.py.)"""
import functools
import types

import numpy as np
import pytest

from bitcmp import same_bits
from kernel_tables import LIM

BIG_FLOATS = LIM // 4 + (1 << 21)   # the NaN buffer an operand beyond the window is a view of


# ---- fixtures -----------------------------------------------------------------------------------------------------------
def handle_fixture(kernel="auto", check_timeouts=False, reset_kernel=False):
    """A module-scoped handle of the module's own on `kernel` (the session fixture `mm` is on `mfma`, which has no op,
    epilogue or batched forms).  check_timeouts: no stream-K hand-over of the module timed out; reset_kernel: back to `auto`
    before the handle closes."""
    @pytest.fixture(scope="module")
    def handle():
        import how_to_optimize_gemm_amd as H
        x = H.MMult(0, kernel)
        yield x
        timeouts = x.streamk_timeouts() if check_timeouts else 0
        if reset_kernel:
            x.set_kernel("auto")
        x.close()
        assert timeouts == 0, timeouts
    return handle


def cus_fixture(handle):
    """The module-scoped `cus`: the compute units of the device, asked of the fixture named `handle`."""
    @pytest.fixture(scope="module")
    def cus(request):
        return request.getfixturevalue(handle).device_info()["cu_count"]
    return cus


@pytest.fixture(scope="module")
def big():
    """The flat NaN buffer an operand beyond (or at the edge of) the window is a strided view of."""
    import torch
    buf = torch.full((BIG_FLOATS,), float("nan"), device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


# ---- operands -----------------------------------------------------------------------------------------------------------
def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def stored(x, t):
    """The operand as mmh_sgemm_op reads it: x itself (op N) or its transpose, materialised (op T)."""
    return np.ascontiguousarray(x.T if t else x)


def _nan_stored(rows, cols, ld, off):
    """A device buffer of `rows` x `cols` values at row stride `ld`, `off` floats into the allocation: NaN in the padding
    of every row, in front of the first row and behind the last one."""
    import torch
    flat = torch.full((off + rows * ld + 64,), float("nan"), device="cuda")
    return flat, flat[off:off + rows * ld].view(rows, ld)


def _padded(rows, cols, ld, off, fill=None):
    """A NaN buffer, and the rows x ld view at `off` floats into it with `fill` in its first `cols` columns."""
    import torch
    flat = torch.full((rows * ld + off + 8,), float("nan"), device="cuda")
    view = flat[off:off + rows * ld].view(rows, ld)
    if fill is not None:
        view[:, :cols] = torch.from_numpy(np.ascontiguousarray(fill)).cuda()
    return flat, view


def _ld(cols, guarded):
    return cols + (1 if cols % 2 == 0 else 2) if guarded else cols + 4   # odd, or a multiple of 4 floats past the row


def _strided(flat, rows, cols, ld, off):
    import torch
    assert off + (rows - 1) * ld + cols <= flat.numel(), ("the operand does not fit its buffer", rows, cols, ld, off, flat.numel())
    return torch.as_strided(flat, (rows, cols), (ld, 1), off)


@functools.lru_cache(maxsize=16)
def _case(m, n, k):
    """Inputs and the oracle's overwrite / accumulate results of one shape (every row that runs it reuses them)."""
    from oracle import oracle as O
    a, b = O.harness_inputs(m, n, k, seed=(31 * m + 7 * n + k) % (1 << 31))
    c0 = np.random.default_rng(m + n + k).uniform(-1, 1, (m, n)).astype(np.float32)
    return a, b, c0, O.ref_mmult(a, b, fma=True), O.ref_mmult(a, b, c0.copy(), fma=True)


# ---- one GEMM on NaN-padded operands --------------------------------------------------------------------------------------
def run_gemm(mm, a, b, c_init, accumulate, guarded, ops=None):
    """C = op(A) op(B) (+ C) through mmh_sgemm / mmh_sgemm_op on NaN-padded operands: guarded -- odd leading dimensions and
    bases 4 bytes past 16-byte alignment; otherwise leading dimensions that are multiples of 4 and 16-byte aligned bases.
    Returns (C's window, whether anything outside it was written, the launch string)."""
    import torch
    import how_to_optimize_gemm_amd as H
    m, k = a.shape
    n = b.shape[1]
    off = 1 if guarded else 4
    ta, tb = ops or (0, 0)
    sa = np.ascontiguousarray(a.T) if ta else a
    sb = np.ascontiguousarray(b.T) if tb else b
    lda, ldb, ldc = _ld(sa.shape[1], guarded), _ld(sb.shape[1], guarded), _ld(n, guarded)
    _, av = _padded(*sa.shape, lda, off, sa)
    _, bv = _padded(*sb.shape, ldb, off, sb)
    cflat, cv = _padded(m, n, ldc, off, c_init)
    s = torch.cuda.current_stream().cuda_stream
    if ops is None:
        mm.sgemm(m, n, k, av.data_ptr(), lda, bv.data_ptr(), ldb, cv.data_ptr(), ldc, accumulate, s)
    else:
        mm.sgemm_op(ta, tb, m, n, k, av.data_ptr(), lda, bv.data_ptr(), ldb, cv.data_ptr(), ldc, accumulate, s)
    launched = H.last_launch()
    torch.cuda.synchronize()
    untouched = bool(torch.isnan(cv[:, n:]).all()) and bool(torch.isnan(cflat[:off]).all()) and \
        bool(torch.isnan(cflat[off + m * ldc:]).all())
    return cv[:, :n].cpu().numpy(), untouched, launched


def run_strided(mm, big, a, b, c_init, accumulate, guarded, lda=0, ldb=0):
    """run_gemm with A (lda given) or B (ldb given) as a view of `big` with that leading dimension; NaN goes back over the
    view afterwards.  Returns (C's window, whether anything outside it was written, the launch string)."""
    import torch
    import how_to_optimize_gemm_amd as H
    if not lda and not ldb:
        return run_gemm(mm, a, b, c_init, accumulate, guarded)
    assert not (lda and ldb), ("one buffer, one large operand", lda, ldb)
    m, k = a.shape
    n = b.shape[1]
    off = 1 if guarded else 4
    ldc = _ld(n, guarded)
    if lda:
        av = _strided(big, m, k, lda, off)
        av.copy_(torch.from_numpy(a))
        ldb = _ld(n, guarded)
        _, bv = _padded(k, n, ldb, off, b)
        view = av
    else:
        bv = _strided(big, k, n, ldb, off)
        bv.copy_(torch.from_numpy(b))
        lda = _ld(k, guarded)
        _, av = _padded(m, k, lda, off, a)
        view = bv
    try:
        cflat, cv = _padded(m, n, ldc, off, c_init)
        mm.sgemm(m, n, k, av.data_ptr(), lda, bv.data_ptr(), ldb, cv.data_ptr(), ldc, accumulate, torch.cuda.current_stream().cuda_stream)
        launched = H.last_launch()
        torch.cuda.synchronize()
        untouched = bool(torch.isnan(cv[:, n:]).all()) and bool(torch.isnan(cflat[:off]).all()) and \
            bool(torch.isnan(cflat[off + m * ldc:]).all())
        return cv[:, :n].cpu().numpy(), untouched, launched
    finally:
        view.fill_(float("nan"))


class _Options:
    """A row's reach on the session handle, and the defaults back afterwards."""

    def __init__(self, mm, inst):
        self.mm, self.inst = mm, inst

    def __enter__(self):
        import how_to_optimize_gemm_amd as H
        self.mm.set_kernel(self.inst.kernel)
        self.mm.set_streamk(self.inst.streamk)
        self.mm.set_option(H.OPT_STREAMK_CHAIN, self.inst.chain)
        self.mm.set_option(H.OPT_PERSIST, self.inst.persist)

    def __exit__(self, *exc):
        import how_to_optimize_gemm_amd as H
        self.mm.set_option(H.OPT_PERSIST, 0)
        self.mm.set_option(H.OPT_STREAMK_CHAIN, 1)
        self.mm.set_streamk(1)
        self.mm.set_kernel("mfma")


def _reach(mm, kernel, streamk=0, persist=0):
    return _Options(mm, types.SimpleNamespace(kernel=kernel, streamk=streamk, chain=1, persist=persist))


# ---- a batch --------------------------------------------------------------------------------------------------------------
class Batch:
    """One batched problem laid out in flat host buffers: each operand's matrices at off + i * stride with leading dimension
    ld (stride 0: one matrix for the whole batch), NaN everywhere else -- ld padding, gaps between matrices, in front of
    the base.  Logical matrices are kept for the oracle."""

    def __init__(self, ta, tb, m, n, k, batch, seed, lda=0, ldb=0, ldc=0, sa=None, sb=None, sc=None, offs=(0, 0, 0),
                 a_val=None, b_val=None, c_val=None):
        rng = np.random.default_rng(seed)
        self.ta, self.tb, self.m, self.n, self.k, self.batch = ta, tb, m, n, k, batch
        ra, ca = (k, m) if ta else (m, k)
        rb, cb = (n, k) if tb else (k, n)
        self.lda, self.ldb, self.ldc = lda or ca, ldb or cb, ldc or n
        self.sa = ra * self.lda if sa is None else sa
        self.sb = rb * self.ldb if sb is None else sb
        self.sc = m * self.ldc if sc is None else sc
        self.offs = offs

        def lay(rows, cols, ld, s, off, fill):
            count = batch if s else 1
            flat = np.full(off + (count - 1) * s + rows * ld + 5, np.nan, np.float32)
            mats = []
            for i in range(count):
                x = fill(rows, cols)
                flat[off + i * s:off + i * s + rows * ld].reshape(rows, ld)[:, :cols] = x
                mats.append(x)
            return flat, mats

        uni = lambda r, c: rng.uniform(-1, 1, (r, c)).astype(np.float32)
        self.a, am = lay(ra, ca, self.lda, self.sa, offs[0], a_val or uni)
        self.b, bm = lay(rb, cb, self.ldb, self.sb, offs[1], b_val or uni)
        self.c0, self.cm = lay(m, n, self.ldc, self.sc, offs[2], c_val or uni)
        self.A = [(x.T if ta else x) for x in am]
        self.B = [(x.T if tb else x) for x in bm]

    def logical(self, i):
        return (np.ascontiguousarray(self.A[i if self.sa else 0]), np.ascontiguousarray(self.B[i if self.sb else 0]))

    def c_window(self, flat, i):
        o = self.offs[2] + i * self.sc
        return flat[o:o + self.m * self.ldc].reshape(self.m, self.ldc)[:, :self.n]

    def want(self, oracle, i, accumulate):
        a, b = self.logical(i)
        c = self.cm[i].copy() if accumulate else None
        return oracle.ref_mmult(a, b, c, fma=True)

    def run(self, h, accumulate=False, stream=None):
        import torch
        da, db, dc = (torch.from_numpy(x).cuda() for x in (self.a, self.b, self.c0))
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        h.sgemm_batched(self.ta, self.tb, self.m, self.n, self.k, da.data_ptr() + 4 * self.offs[0], self.lda, self.sa,
                        db.data_ptr() + 4 * self.offs[1], self.ldb, self.sb, dc.data_ptr() + 4 * self.offs[2], self.ldc, self.sc,
                        self.batch, accumulate, s)
        torch.cuda.synchronize()
        return dc.cpu().numpy()

    def check(self, oracle, got, accumulate, what):
        inside = np.zeros(got.shape, dtype=bool)
        for i in range(self.batch):
            assert same_bits(self.c_window(got, i), self.want(oracle, i, accumulate)), (what, "matrix", i)
            o = self.offs[2] + i * self.sc
            inside[o:o + self.m * self.ldc].reshape(self.m, self.ldc)[:, :self.n] = True
        assert same_bits(got[~inside], self.c0[~inside]), (what, "wrote outside the C matrices")
