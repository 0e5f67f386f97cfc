"""Every int8 GEMM and quantiser instantiation of libmmult_hip.so against an exact reference.

INSTANTIATIONS has one row per instantiation of the int8 side (BASELINE config 5): the correctness-first kernel
igemm_s8_simple_kernel, K3t igemm_s8_dma_kernel (B read in place), K3p igemm_s8_pp_kernel (ping-pong, persistent;
with and without the dequantising epilogue, on the 64- and the 32-deep MFMA), and the quantiser passes absmax_kernel,
quantize_kernel and dequantize_kernel.  A row says how a caller reaches its instantiation (entry point and
MMH_OPT_IGEMM_MODE), and the shapes it runs; the launchers' host arithmetic is restated in tests/int8_ops.py (`reach`, with
the Case vocabulary and the functions that run and compare one call), and the words of
mmh_last_launch prove that the instantiation ran.  tests/test_int8_coverage.py holds the table to the symbols of the built
library and every case to its row's instantiation, on the CPU.

The reference of the GEMM is a.astype(float64) @ b.astype(float64) (+ C0): exact here, every partial sum is an integer
below 2^53.  It is compared as int64, and asserted separately to fit in int32 (the oracle's int32 loop would wrap without
a word).  The quantiser is compared bit for bit with oracle.quantize_sym_s8, qgemm with acc * (1 / (sa * sb)) on the
oracle's integers and scales.  Everything outside C's window is a guard value that must survive."""
import dataclasses
import os
import subprocess
import sys
from typing import Callable, Optional

import numpy as np
import pytest

from built_lib import REPO
from int8_ops import (GUARD_I8, INT32_MAX, Case, _big_side, _buffer, _cus, _int8, _window, pp_grid, reach, reference,
                      run_case, run_igemm_view)

pytestmark = pytest.mark.gpu

KS = (1, 3, 4, 63, 64, 65, 127, 128, 129, 255, 256, 257)   # a slice is 128 bytes; K3t rounds the slice count up to even
THIN = (1, 3, 4, 5, 15, 16, 17)                           # last tiles: C stores go in 4 columns, the transposer in 16 rows


# ---- the table ----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Inst:
    symbol: str                       # as tools/kernel_resources.py demangles it
    entry: str                        # "igemm" (mmh_igemm_s8), "qgemm" (mmh_qgemm_f32), "quantize" (mmh_quantize_sym_s8)
    mode: int                         # MMH_OPT_IGEMM_MODE
    cases: Callable                   # cus -> [Case]
    worst: Optional[Callable] = None  # cus -> the one-tile Case of all -128 x all -128 at the deepest k that fits int32
    persistent: bool = False          # walks several tiles per workgroup under MMH_I8_GRID_CAP (a child process)


def _pad4(x):
    return x + (-x % 4)


def _whole(t, ks=KS, align=4):
    """Whole tiles on every K-tail class; leading dimensions padded (in-place kernels: multiples of 4, the simple kernel's
    unguarded form: of 16), C windows with ldc = n + 4 and a base 16 bytes off."""
    def cases(cus):
        out = []
        for i, k in enumerate(ks):
            m, n = t * (1 + i % 3), t * (1 + (i + 1) % 2)
            ka = k + (-k % align)
            out.append(Case(m, n, k, lda=ka + align * (i % 3), ldb=n + 4 * (i % 3), ldc=n + 4 * (i % 2), oc=4 * (i % 2)))
        return out
    return cases


def _ragged(t):
    """Last tiles of 1, 3, 4, 5, 15, 16, 17 rows and columns on every K-tail class; C windows with ldc = n + 1 / n + 3 and a
    base one int32 off (EDGE on whole tiles, with unaligned vector stores); dword leading dimensions, some padded."""
    def cases(cus):
        out = []
        for i, k in enumerate(KS):
            m = t + THIN[i % len(THIN)] + (t if i % 5 == 4 else 0)
            n = t * ((i + 1) % 2) + THIN[(i + 2) % len(THIN)]
            out.append(Case(m, n, k, lda=_pad4(k) + 4 * (i % 2), ldb=_pad4(n) + (8 if i % 3 == 0 else 0),
                            ldc={1: n + 1, 3: n + 3}.get(i % 4, 0), oc=1 if i % 4 == 1 else 0))
        out += [Case(t, t, 129, lda=132, ldc=t + 1, oc=1), Case(2 * t, t, 64, ldc=t + 3), Case(t, 2 * t, 200, oc=1),
                Case(1, 4, 4), Case(1, 5, 256, ldb=8)]
        return out
    return cases


def _misaligned(t):
    """Odd leading dimensions and A / B bases 1, 2, 3 bytes off: the workspace copies of mode 0."""
    def cases(cus):
        return [Case(t + 5, t - 3, 67, lda=71, ob=2, mode=0), Case(t - 1, t + 17, 130, oa=1, ldb=t + 20, mode=0),
                Case(2 * t + 3, 15, 255, lda=259, ldb=17, oa=3, ob=1, mode=0)]
    return cases


def _simple_edge(cus):
    return _ragged(128)(cus) + [Case(131, 133, 67, lda=67, ldb=133, oa=1, ob=2, oc=1, ldc=135), Case(128, 128, 128, oa=3),
                                Case(257, 130, 255, lda=258, ldb=131, ob=3, ldc=131), Case(3, 1, 1)]


def _k3t_edge(t):
    def cases(cus):
        return _ragged(t)(cus) + (_misaligned(t)(cus) if t == 128 else [])
    return cases


def _pp_edge(mode):
    """K3p's guarded rows; the 64-deep one also in mode 9 (the same instantiation, one workgroup per tile)."""
    def cases(cus):
        m9 = 9 if mode == 8 else None
        return _ragged(256)(cus) + [Case(300, 700, 1000, mode=m9), Case(257, 255, 129, lda=132, ldb=256, ldc=256, oc=1, mode=m9)]
    return cases


def _deq(edge):
    """qgemm's fused path on the 256x256 tile (the default rule picks it only at several tiles per CU)."""
    def cases(cus):
        s = _big_side(cus)
        if not edge:
            return [Case(s, s, 64), Case(s, s + 256, 129, ldc=s + 260), Case(s, s, 3, lda=8, ldb=s + 4)]
        return [Case(s - 5, s + 3, 257), Case(s, s, 65, ldc=s + 1, oc=1), Case(s + 17, s - 255, 1, lda=5, ob=1)]
    return cases


def _worst(t, edge, mode, k=131071):
    """One tile of all -128 x all -128: k * 16384 = 2,147,467,264 at k = 131071 (simple<false>: k % 64 == 0)."""
    def case(cus):
        return Case(t - 1 if edge else t, t - 4 if edge else t, k, lda=_pad4(k), mode=mode)
    return case


def _quant_paths(cus):
    """Both paths of both passes: cols 1 .. 5 and 4097 with ld = cols and ld padded to a multiple of 4, bases 0 and one
    float off; 7 rows (chunk counts that are not a multiple of QG) and 301 (more than AMAX_WORDS workgroups)."""
    out = []
    for cols in (1, 2, 3, 4, 5, 4097):
        for ld in (cols, cols + (-cols % 4) + 4):
            for off in (0, 1):
                out.append(Case(7 if (cols + off) % 2 else 301, cols, lda=ld, oa=off))
    out += [Case(1, 3), Case(1, 4097, oa=1), Case(4099, 2, lda=4)]
    return out


def _quant_values(cus):
    """Exact .5 ties after scaling (round half to even), -0.0, +-max|x| itself; and qgemm's lopsided pairs, whose surplus
    workgroups of the smaller tensor exit, among them the 1 - 3 column windows of a 16-byte aligned, ld % 4 == 0 tensor."""
    return [Case(9, 33, values="ties"), Case(300, 129, lda=132, values="ties"), Case(1, 4, values="ties"),
            Case(4096, 3, 8, entry="qgemm", mode=0), Case(4096, 3, 8, ldb=4, entry="qgemm", mode=0),
            Case(300, 64, 2, lda=4, entry="qgemm", mode=0), Case(3, 4096, 8, lda=12, entry="qgemm", mode=0),
            Case(1000, 1, 300, ldb=4, ldc=5, oc=1, entry="qgemm", mode=0),
            Case(517, 259, 97, lda=100, ldb=263, oa=1, ob=4, ldc=262, oc=2, entry="qgemm", mode=0)]


def _dequant(cus):
    """The two-pass form (int32 C in workspace, then dequantize_kernel): strided inputs, a strided C window."""
    return [Case(4096, 3, 8, ldb=4, mode=5), Case(300, 64, 2, lda=4, mode=2), Case(333, 257, 129, mode=5),
            Case(517, 259, 97, lda=100, ldb=263, oa=1, ob=4, ldc=262, oc=2, mode=2), Case(3, 4096, 8, lda=12, mode=6),
            Case(1, 1, 1, mode=5)]


INSTANTIATIONS = [
    Inst("igemm_s8_simple_kernel<false>", "igemm", 2, _whole(128, ks=(64, 128, 192, 256, 320), align=16),
         worst=_worst(128, False, 2, k=131008)),
    Inst("igemm_s8_simple_kernel<true>", "igemm", 2, _simple_edge, worst=_worst(128, True, 2)),
    Inst("igemm_s8_dma_kernel<128,128,4,false,0,true>", "igemm", 5, _whole(128), worst=_worst(128, False, 5)),
    Inst("igemm_s8_dma_kernel<128,128,4,true,0,true>", "igemm", 5, _k3t_edge(128), worst=_worst(128, True, 5)),
    Inst("igemm_s8_dma_kernel<256,256,8,false,0,true>", "igemm", 6, _whole(256), worst=_worst(256, False, 6)),
    Inst("igemm_s8_dma_kernel<256,256,8,true,0,true>", "igemm", 6, _k3t_edge(256), worst=_worst(256, True, 6)),
    Inst("igemm_s8_pp_kernel<false,false,64>", "igemm", 8, _whole(256), worst=_worst(256, False, 8), persistent=True),
    Inst("igemm_s8_pp_kernel<true,false,64>", "igemm", 8, _pp_edge(8), worst=_worst(256, True, 8), persistent=True),
    Inst("igemm_s8_pp_kernel<false,true,64>", "qgemm", 0, _deq(False), persistent=True),
    Inst("igemm_s8_pp_kernel<true,true,64>", "qgemm", 0, _deq(True), persistent=True),
    Inst("igemm_s8_pp_kernel<false,false,32>", "igemm", 7, _whole(256), worst=_worst(256, False, 7), persistent=True),
    Inst("igemm_s8_pp_kernel<true,false,32>", "igemm", 7, _pp_edge(7), worst=_worst(256, True, 7), persistent=True),
    Inst("absmax_kernel", "quantize", 0, _quant_paths),
    Inst("quantize_kernel", "quantize", 0, _quant_values),
    Inst("dequantize_kernel", "qgemm", 5, _dequant),
]

# the K3p walks run in a child process with MMH_I8_GRID_CAP = GRID_CAP (read at mmh_create): 8 workgroups walk the tiles
GRID_CAP = 8


def _persistent_cases(inst, cus):
    """Several tiles per workgroup: whole and ragged grids (a ragged last tile), k short enough that a tile's stores are
    still in flight when the next tile ends."""
    edge = inst.symbol.startswith("igemm_s8_pp_kernel<true,")
    if inst.entry == "qgemm":
        return _deq(edge)(cus)[:2]
    if not edge:
        return [Case(1536, 1280, 257, lda=260), Case(2048, 768, 64, ldc=772), Case(1024, 1024, 640)]
    return [Case(1283, 1027, 129, lda=132, ldb=1028), Case(1536, 1280, 63, lda=64, ldc=1281, oc=1),
            Case(1280, 1533, 300, lda=304, ldb=1536)]


# ---- the tests ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=lambda i: i.symbol)
def test_every_int8_instantiation_is_exact(mm, inst):
    """Every row's cases, overwrite and accumulate, bit for bit, C's surroundings untouched, the marker its symbol's."""
    cus = _cus()
    rng = np.random.default_rng(sum(map(ord, inst.symbol)))
    for c in inst.cases(cus):
        assert inst.symbol in run_case(mm, inst, c, rng, cus), (inst.symbol, c)


@pytest.mark.parametrize("inst", [i for i in INSTANTIATIONS if i.worst], ids=lambda i: i.symbol)
def test_worst_case_magnitude_fits_and_is_exact(mm, inst):
    """All -128 x all -128 on one tile at the deepest k that fits: 131071 * 16384 = 2,147,467,264; accumulated onto
    INT32_MAX - that, every element must be exactly INT32_MAX."""
    import torch
    import how_to_optimize_gemm_amd as H
    c = inst.worst(_cus())
    lda, ldb, ldc = c.lds("igemm")
    _, av = _buffer(c.m, c.k, lda, 0, torch.int8, GUARD_I8)
    _, bv = _buffer(c.k, c.n, ldb, 0, torch.int8, GUARD_I8)
    av.fill_(-128)
    bv.fill_(-128)
    total = int(reference(np.full((1, c.k), -128, np.int8), np.full((c.k, 1), -128, np.int8))[0, 0])
    assert total == 16384 * c.k and total <= INT32_MAX
    mm.set_igemm_mode(c.mode)
    try:
        out = mm.igemm_s8(av, bv)
        torch.cuda.synchronize()
        assert inst.symbol in H.last_launch(), H.last_launch()
        assert int(out.min()) == int(out.max()) == total, (inst.symbol, int(out.min()), int(out.max()))
        out.fill_(INT32_MAX - total)
        mm.igemm_s8(av, bv, out=out, accumulate=True)
        assert int(out.min()) == int(out.max()) == INT32_MAX, (inst.symbol, int(out.min()), int(out.max()))
    finally:
        mm.set_igemm_mode(0)


def _persistent_walks():
    """Runs in a child process with MMH_I8_GRID_CAP set: every persistent row walks several tiles per workgroup."""
    sys.path.insert(0, REPO)
    import how_to_optimize_gemm_amd as H
    cus = _cus()
    cap = int(os.environ["MMH_I8_GRID_CAP"])
    mm = H.MMult(0)
    try:
        runs = 0
        for inst in INSTANTIATIONS:
            if not inst.persistent:
                continue
            rng = np.random.default_rng(len(inst.symbol))
            for c in _persistent_cases(inst, cus):
                tiles, grid = pp_grid(c.m, c.n, cap)
                assert grid < tiles, (inst.symbol, c)
                assert inst.symbol in run_case(mm, inst, c, rng, cus, env_cap=cap, words=("persistent",)), (inst.symbol, c)
                runs += 1
        print(f"persistent walks: {runs} cases")
    finally:
        mm.close()


def test_persistent_walks_in_a_child_process():
    """K3p with a small persistent grid (MMH_I8_GRID_CAP, read at mmh_create: set in a fresh child, never here): the next
    tile's prologue goes out in front of the finished tile's C stores -- ragged last tiles, accumulate, the DEQ epilogue."""
    env = dict(os.environ, MMH_I8_GRID_CAP=str(GRID_CAP))
    code = f"import sys; sys.path.insert(0, {os.path.join(REPO, 'tests')!r}); import test_gpu_int8_parity as T; T._persistent_walks()"
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "persistent walks:" in r.stdout, r.stdout


def test_b_beyond_the_descriptor_window_takes_the_simple_kernel(mm):
    """ldb = 2^24 at k = 160: B spans 2.5 GiB, past the 2 GiB window of the buffer descriptors -> the simple kernel, in
    place with 64-bit addresses, in the default mode."""
    import torch
    import how_to_optimize_gemm_amd as H
    rng = np.random.default_rng(24)
    m, n, k, ldb = 300, 133, 160, 1 << 24
    c = Case(m, n, k, ldb=ldb)
    assert reach("igemm", 0, c, _cus())[0] == ["igemm_s8_simple_kernel<true>"]
    a, b = _int8(rng, (m, k)), _int8(rng, (k, n))
    flat = torch.full(((k - 1) * ldb + n,), GUARD_I8, dtype=torch.int8, device="cuda")
    bv = _window(flat, k, n, ldb, 0)
    bv.copy_(torch.from_numpy(b))
    try:
        out = mm.igemm_s8(torch.from_numpy(a).cuda(), bv)
        torch.cuda.synchronize()
        assert "igemm_s8_simple_kernel<true>" in H.last_launch(), H.last_launch()
        assert np.array_equal(out.cpu().numpy().astype(np.int64), reference(a, b))
    finally:
        del flat, bv
        torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", [0, 5, 6, 8])
def test_a_larger_than_4_gib_stays_in_place(mm, mode):
    """A as a (36000, 131072) int8 view -- 4.4 GiB -- with k = 67: in place (lda keeps a tile's offsets inside the window),
    so the tiles past 4 GiB rely on the per-tile descriptor base A + row0 * lda."""
    import torch
    rng = np.random.default_rng(40 + mode)
    m, n, k, lda = 36000, 260, 67, 131072
    big = torch.empty((m, lda), dtype=torch.int8, device="cuda")
    try:
        a, b = _int8(rng, (m, k)), _int8(rng, (k, n))
        big[:, :k] = torch.from_numpy(a).cuda()
        big[:, k:k + 61].fill_(GUARD_I8)                      # what a stray read past k would pick up
        c = Case(m, n, k, lda=lda)
        syms, _ = reach("igemm", mode, c, _cus())
        assert "simple" not in syms[0], syms
        got = run_igemm_view(mm, mode, big[:, :k], b, syms)
        assert np.array_equal(got.astype(np.int64), reference(a, b)), mode
    finally:
        del big
        torch.cuda.empty_cache()
