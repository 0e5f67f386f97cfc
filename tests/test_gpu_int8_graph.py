"""The int8 and quantised calls under graph capture and scratch growth.  mmh_igemm_s8, mmh_quantize_sym_s8 and mmh_qgemm_f32
keep int8 images (qa, qb), an int32 image (qc, the two-pass form) and abs-max words and scales (qs) in per-handle scratch that
grows on demand.  Here: every form captured into a hipGraph replays the parity module's contract on new inputs; a captured call
that would have to allocate or grow its scratch is refused before anything is recorded and disturbs nothing; a graph survives
later growth (the buffers it points at are retired -- counted by MMH_OPT_RETIRED_BUFFERS, which is asserted BEFORE any replay, so
a build that frees under the graph fails at the counter and never replays a dangling graph); two handles on two streams overlap;
and bytes left in the scratch by an earlier, larger call never reach a later result.

The references are tests/int8_ops.py's: oracle.quantize_sym_s8 bit for bit, exact integer sums, float32(acc) * (1 / (sa * sb)).
Every capture is on one side stream after one eager call of each shape on that stream: no graph here has parallel branches, and
no first-ever launch is captured.

What the replays found: the abs-max words were zeroed by a hipMemsetAsync node, and from the SECOND replay of a graph on that
node filled them with a stale pattern above every real maximum (the first replay was exact, and so was every eager call) -- a
captured mmh_quantize_sym_s8 with max|x| = 100, 60, 80, 40, 90 over five replays gave the scales 127 / 100, then 127 / 2^59 four
times.  The words are now zeroed by a device copy of a zero block (csrc/igemm.hip, zero_amax); three replays on new data per
form are what holds that."""
import ctypes
import gc

import numpy as np
import pytest

from gpu_operands import handle_fixture
from int8_ops import (GUARD_F32, GUARD_I8, GUARD_I32, Case, _big_side, _buffer, _check_c, _cus, _int8, _quant_input, inplace_ok,
                      reach, reference, run_igemm, run_qgemm, run_quantize)

pytestmark = pytest.mark.gpu

amm = handle_fixture()   # the module's own handle for the replay tests; the growth and refusal tests make theirs

# the parity table's shapes
RAGGED = Case(517, 259, 97, lda=100, ldb=263, oa=1, ob=4, ldc=262, oc=2)
COLUMN = Case(1000, 1, 300, ldb=4, ldc=5, oc=1)
THIN_K = Case(300, 64, 2, lda=4)
MID = Case(333, 257, 129)
MISALIGNED = (Case(133, 125, 67, lda=71, ob=2), Case(127, 145, 130, oa=1, ldb=148), Case(259, 15, 255, lda=259, ldb=17, oa=3, ob=1))
MISALIGNED_LARGE = Case(261, 253, 67, lda=71, ob=2)   # _misaligned(256)'s first: both images larger than MISALIGNED[0]'s
# The two-pass refusal must come from qc ALONE (qa and qb fit, so only the order of the checks can tell): a deep, narrow shape
# first -- qa = qb = 64 x 2048 bytes, qc = 64 x 64 x 4 -- then MID, whose images are smaller and whose qc is 333 x 260 x 4.
DEEP = Case(64, 64, 2048)


# ---- one call, its operands and its reference -----------------------------------------------------------------------------
class _Op:
    """A call on fixed device buffers: fill() writes new inputs in place and the guard value over the outputs, call() issues
    the call (eagerly or into a capture) and holds its launch marker to `reach`, check() compares with the reference."""
    entry = None

    def __init__(self, c, mode=0):
        self.c, self.mode = c, mode

    def marker(self, launched):
        syms, words = reach(self.entry, self.mode, self.c, _cus())
        for w in list(syms) + list(words):
            assert w in launched, f"{self.entry} mode {self.mode} {self.c}: '{w}' not in the launch marker: {launched}"


class _Qgemm(_Op):
    entry = "qgemm"

    def __init__(self, c, mode=0, saturate=False):
        import torch
        super().__init__(c, mode)
        lda, ldb, ldc = c.lds("qgemm")
        self.saturate = saturate
        _, self.av = _buffer(c.m, c.k, lda, c.oa, torch.float32, 1e30)
        _, self.bv = _buffer(c.k, c.n, ldb, c.ob, torch.float32, -1e30)
        self.cflat, self.cv = _buffer(c.m, c.n, ldc, c.oc, torch.float32, GUARD_F32)

    def fill(self, rng):
        import torch
        c = self.c
        if self.saturate:   # every |x| is the maximum: every byte of the int8 images is +-127
            self.a = np.where(rng.random((c.m, c.k)) < 0.5, -1.5, 1.5).astype(np.float32)
            self.b = np.where(rng.random((c.k, c.n)) < 0.5, -0.25, 0.25).astype(np.float32)
        else:
            self.a = rng.uniform(-2, 2, (c.m, c.k)).astype(np.float32)
            self.b = rng.uniform(-0.5, 0.5, (c.k, c.n)).astype(np.float32)
        self.av.copy_(torch.from_numpy(self.a))
        self.bv.copy_(torch.from_numpy(self.b))
        self.cflat.fill_(GUARD_F32)

    def call(self, mm):
        import how_to_optimize_gemm_amd as H
        mm.set_igemm_mode(self.mode)
        try:
            mm.qgemm(self.av, self.bv, out=self.cv)
            self.marker(H.last_launch())
        finally:
            mm.set_igemm_mode(0)

    def check(self, what):
        from oracle import oracle as O
        qa, sa = O.quantize_sym_s8(self.a)
        qb, sb = O.quantize_sym_s8(self.b)
        if self.saturate:
            assert np.abs(qa).min() == 127 and np.abs(qb).min() == 127
        inv = np.float32(1.0) / (np.float32(sa) * np.float32(sb))
        _check_c(self.cflat, self.cv, reference(qa, qb).astype(np.float32) * inv, GUARD_F32, f"{what}: qgemm mode {self.mode} {self.c}")

    def untouched(self):
        return bool((self.cflat == GUARD_F32).all())


class _Quantize(_Op):
    entry = "quantize"

    def __init__(self, c):
        import torch
        super().__init__(c)
        ld, _, _ = c.lds("quantize")
        _, self.xv = _buffer(c.m, c.n, ld, c.oa, torch.float32, 1e30)
        self.q = self.s = None

    def fill(self, rng):
        import torch
        self.x = _quant_input(rng, self.c.m, self.c.n, self.c.values)
        self.xv.copy_(torch.from_numpy(self.x))
        if self.q is not None:
            self.q.fill_(GUARD_I8)
            self.s.fill_(GUARD_F32)

    def call(self, mm):
        import how_to_optimize_gemm_amd as H
        self.q, self.s = mm.quantize_sym_s8(self.xv)   # (captured: tensors of the graph's pool, held here)
        self.marker(H.last_launch())

    def check(self, what):
        from oracle import oracle as O
        q_ref, s_ref = O.quantize_sym_s8(self.x)
        got = self.q.cpu().numpy()
        assert np.float32(self.s.item()).view(np.uint32) == np.float32(s_ref).view(np.uint32), (what, self.c, self.s.item(), s_ref)
        assert np.array_equal(got, q_ref), f"{what}: quantize {self.c}: {int((got != q_ref).sum())} of {got.size} q differ"


class _Igemm(_Op):
    entry = "igemm"

    def __init__(self, c, mode=0, accumulate=False, fill_value=None):
        import torch
        super().__init__(c, mode)
        lda, ldb, ldc = c.lds("igemm")
        self.accumulate, self.fill_value = accumulate, fill_value
        _, self.av = _buffer(c.m, c.k, lda, c.oa, torch.int8, GUARD_I8)
        _, self.bv = _buffer(c.k, c.n, ldb, c.ob, torch.int8, -GUARD_I8)
        self.cflat, self.cv = _buffer(c.m, c.n, ldc, c.oc, torch.int32, GUARD_I32)

    def fill(self, rng):
        import torch
        c = self.c
        if self.fill_value is None:
            self.a, self.b = _int8(rng, (c.m, c.k)), _int8(rng, (c.k, c.n))
        else:
            self.a, self.b = np.full((c.m, c.k), self.fill_value, np.int8), np.full((c.k, c.n), self.fill_value, np.int8)
        self.c0 = rng.integers(-(1 << 20), 1 << 20, (c.m, c.n), dtype=np.int32) if self.accumulate else None
        self.av.copy_(torch.from_numpy(self.a))
        self.bv.copy_(torch.from_numpy(self.b))
        self.cflat.fill_(GUARD_I32)
        if self.accumulate:
            self.cv.copy_(torch.from_numpy(self.c0))

    def call(self, mm):
        import how_to_optimize_gemm_amd as H
        mm.set_igemm_mode(self.mode)
        try:
            mm.igemm_s8(self.av, self.bv, out=self.cv, accumulate=self.accumulate)
            self.marker(H.last_launch())
        finally:
            mm.set_igemm_mode(0)

    def check(self, what):
        _check_c(self.cflat, self.cv, reference(self.a, self.b, self.c0), GUARD_I32,
                 f"{what}: igemm mode {self.mode} {self.c} {'accumulate' if self.accumulate else 'overwrite'}")

    def untouched(self):
        return bool((self.cflat == GUARD_I32).all())


# ---- capture and replay ---------------------------------------------------------------------------------------------------
def _side_stream():
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    return side


def _eager(mm, side, ops, rng, what="eager"):
    """One uncaptured call of each op on `side` (torch's warm-up rule: it sizes the scratch), checked."""
    import torch
    for op in ops:
        op.fill(rng)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for op in ops:
            op.call(mm)
    side.synchronize()
    for op in ops:
        op.check(what)


def _capture(side, body):
    """The graph of body() captured on `side`.  No CUDAGraph may die while a stream is capturing: destroying one there took the
    whole pytest process down (an abort inside the collector, which _captured_nodes' set of thousands of strings tends to start
    during the capture).  `del graph` does not free the graph of a body that keeps its `pytest.raises(...) as e`: e holds the
    traceback, that holds body's frame and through f_back this frame and its `graph` -- a dead cycle only the collector frees,
    at a time of its choosing.  So such bodies end with `del e`, and whatever other tests left behind is collected here, before
    the capture begins (torch.cuda.graph did that itself until it became an option)."""
    import torch
    gc.collect()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            body()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def _replays(graph, ops, rng, count):
    import torch
    for rep in range(count):
        for op in ops:
            op.fill(rng)
        graph.replay()
        torch.cuda.synchronize()
        for op in ops:
            op.check(f"replay {rep}")


def _replays_the_contract(mm, ops, seed):
    """One graph of `ops` on a side stream, after one eager call of each; three replays on fresh data."""
    rng = np.random.default_rng(seed)
    side = _side_stream()
    _eager(mm, side, ops, rng)
    graph = _capture(side, lambda: [op.call(mm) for op in ops])
    _replays(graph, ops, rng, 3)
    del graph


def _captured_nodes(side):
    """How many nodes the capture on `side` has recorded so far (two queries of the HIP runtime this process runs on)."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    hip = ctypes.CDLL(paths.pop())
    status, ident, graph, deps, ndeps = ctypes.c_int(0), ctypes.c_ulonglong(0), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(0)
    rc = hip.hipStreamGetCaptureInfo_v2(ctypes.c_void_p(side.cuda_stream), ctypes.byref(status), ctypes.byref(ident),
                                        ctypes.byref(graph), ctypes.byref(deps), ctypes.byref(ndeps))
    assert rc == 0 and status.value == 1 and graph.value, (rc, status.value)   # 1: hipStreamCaptureStatusActive
    count = ctypes.c_size_t(0)
    rc = hip.hipGraphGetNodes(graph, None, ctypes.byref(count))
    assert rc == 0, rc
    return count.value


def scratch_bytes(op):
    """igemm.hip's sizes of the images a call keeps in the handle: qa / qb (quantised, or copied because misaligned), qc (the
    int32 image of the two-pass form).  qs has one size for every call."""
    c = op.c
    lda, ldb, _ = c.lds(op.entry)
    if op.entry == "qgemm":
        ka, nb = (c.k + 15) & ~15, (c.n + 3) & ~3
        need = {"qa": c.m * ka, "qb": c.k * nb}
        if not (op.mode == 0 and inplace_ok(ka, 0, nb, 0, c.k)):
            need["qc"] = 4 * c.m * nb
        return need
    assert op.entry == "igemm" and op.mode == 0
    need = {}
    if lda % 4 or c.oa % 4:
        need["qa"] = c.m * ((c.k + 15) & ~15)
    if ldb % 4 or c.ob % 4:
        need["qb"] = c.k * ((c.n + 15) & ~15)
    return need


def grown(small, large):
    have, want = scratch_bytes(small), scratch_bytes(large)
    return sum(1 for name, size in want.items() if size > have.get(name, 0))


# ---- each form replays the contract on new inputs ---------------------------------------------------------------------------
def test_a_captured_fused_qgemm_on_k3t_replays_the_contract(amm):
    op = _Qgemm(RAGGED)
    assert "igemm_s8_dma_kernel<128,128,4,true,0,true>" in reach("qgemm", 0, RAGGED, _cus())[0]
    _replays_the_contract(amm, [op], 11)


@pytest.mark.parametrize("ragged", [False, True], ids=["whole", "ragged"])
@pytest.mark.parametrize("k", [64, 129])
def test_a_captured_fused_qgemm_on_k3p_replays_the_contract(amm, k, ragged):
    s = _big_side(_cus())
    c = Case(s - 5, s + 3, k, ldc=s + 4, oc=1) if ragged else Case(s, s, k)
    assert f"igemm_s8_pp_kernel<{'true' if ragged else 'false'},true,64>" in reach("qgemm", 0, c, _cus())[0]
    _replays_the_contract(amm, [_Qgemm(c)], 12 + k + ragged)


def test_a_captured_two_pass_qgemm_replays_the_contract(amm):
    """Mode 5: the int32 image qc and dequantize_kernel."""
    ops = [_Qgemm(MID, mode=5), _Qgemm(Case(4096, 3, 8, ldb=4), mode=5)]
    for op in ops:
        assert "dequantize_kernel" in reach("qgemm", 5, op.c, _cus())[0]
    _replays_the_contract(amm, ops, 13)


def test_a_captured_quantize_replays_the_contract_on_both_paths(amm):
    ops = [_Quantize(Case(301, 4097, lda=4100)), _Quantize(Case(7, 5, lda=12, oa=1)), _Quantize(Case(300, 129, lda=132, values="ties"))]
    words = [reach("quantize", 0, op.c, 256)[1] for op in ops]
    assert words[0] == ["absmax_kernel (vector path)", "quantize_kernel (row path)"] and "absmax_kernel (row path)" in words[1]
    assert words[2] == ["absmax_kernel (vector path)", "quantize_kernel (row path)"]
    ops.append(_Quantize(Case(9, 32, values="ties")))                       # both passes on the vector path
    assert reach("quantize", 0, ops[3].c, 256)[1] == ["absmax_kernel (vector path)", "quantize_kernel (vector path)"]
    _replays_the_contract(amm, ops, 14)


def test_a_captured_igemm_in_place_replays_the_contract(amm):
    """Mode 8 (persistent K3p) on a ragged and a whole-tile shape, mode 5 (K3t); overwrite and accumulate."""
    ops = [_Igemm(Case(300, 700, 1000), mode=8), _Igemm(Case(300, 700, 1000), mode=8, accumulate=True),
           _Igemm(Case(512, 256, 129, lda=132), mode=8), _Igemm(Case(512, 256, 129, lda=132), mode=8, accumulate=True),
           _Igemm(Case(131, 133, 257, lda=260, ldb=136, ldc=134, oc=1), mode=5),
           _Igemm(Case(131, 133, 257, lda=260, ldb=136, ldc=134, oc=1), mode=5, accumulate=True)]
    assert reach("igemm", 8, ops[0].c, _cus())[0] == ["igemm_s8_pp_kernel<true,false,64>"]
    assert reach("igemm", 8, ops[2].c, _cus())[0] == ["igemm_s8_pp_kernel<false,false,64>"]
    assert reach("igemm", 5, ops[4].c, _cus())[0] == ["igemm_s8_dma_kernel<128,128,4,true,0,true>"]
    _replays_the_contract(amm, ops, 15)


def test_a_captured_igemm_on_the_workspace_copy_path_replays_the_contract(amm):
    ops = [_Igemm(c, accumulate=acc) for c in MISALIGNED for acc in (False, True)]
    for op in ops:
        assert any("copied to workspace" in w for w in reach("igemm", 0, op.c, _cus())[1]), op.c
    _replays_the_contract(amm, ops, 16)


def test_a_quantize_and_a_qgemm_in_one_graph_use_different_words_of_the_scratch(amm):
    """The stand-alone quantiser's abs-max words lie behind the quantised GEMM's words and scales in qs."""
    ops = [_Quantize(Case(301, 129, lda=132)), _Qgemm(RAGGED), _Quantize(Case(9, 33, values="ties")), _Qgemm(THIN_K)]
    _replays_the_contract(amm, ops, 17)


# ---- a captured call that would grow is refused and disturbs nothing --------------------------------------------------------
def _refused_and_disturbs_nothing(small, large, seed):
    """On a handle that has only run `small`: inside the capture `small` is recorded and `large` is refused with nothing
    recorded; the replay gives small's bits and leaves large's outputs alone; nothing was retired; `large`, uncaptured, then
    grows the scratch and is exact."""
    import torch
    import how_to_optimize_gemm_amd as H
    assert grown(small, large) > 0
    rng = np.random.default_rng(seed)
    with H.MMult(0, "auto") as own:
        side = _side_stream()
        _eager(own, side, [small], rng)
        small.fill(rng), large.fill(rng)
        nodes = []

        def body():
            small.call(own)
            nodes.append(_captured_nodes(side))
            with pytest.raises(H.MMultError) as e:
                large.call(own)
            nodes.append(_captured_nodes(side))
            nodes.append(e.value.status)
            del e   # (see _capture)

        graph = _capture(side, body)
        assert nodes[2] == H.ERR_UNSUPPORTED
        assert nodes[0] > 0 and nodes[1] == nodes[0], f"the refused call recorded {nodes[1] - nodes[0]} nodes"
        graph.replay()
        torch.cuda.synchronize()
        small.check("replay beside a refused call")
        assert large.untouched()
        assert own.get_option(H.OPT_RETIRED_BUFFERS) == 0
        _eager(own, side, [large], rng, "uncaptured after the refusal")   # the handle is not poisoned
        assert own.get_option(H.OPT_RETIRED_BUFFERS) == grown(small, large)   # (before the graph is replayed again)
        _replays(graph, [small], rng, 1)
        del graph


def test_a_captured_fused_qgemm_that_would_grow_is_refused_and_disturbs_nothing():
    _refused_and_disturbs_nothing(_Qgemm(THIN_K), _Qgemm(RAGGED), 21)


def test_a_captured_two_pass_qgemm_is_refused_before_its_quantise_launches():
    """qa, qb and qs are large enough for the refused call, only qc is not: a check of qc that sat behind the abs-max and
    quantise launches would leave those in the graph."""
    small, large = _Qgemm(DEEP, mode=5), _Qgemm(MID, mode=5)
    have, want = scratch_bytes(small), scratch_bytes(large)
    assert want["qa"] <= have["qa"] and want["qb"] <= have["qb"] and want["qc"] > have["qc"]
    _refused_and_disturbs_nothing(small, large, 22)


def test_a_captured_igemm_copy_that_would_grow_is_refused_and_disturbs_nothing():
    _refused_and_disturbs_nothing(_Igemm(MISALIGNED[0]), _Igemm(MISALIGNED_LARGE), 23)


def test_a_handle_without_scratch_refuses_a_captured_quantize():
    """qs does not exist before a handle's first int8 call: nothing can allocate it while the stream is capturing."""
    import torch
    import how_to_optimize_gemm_amd as H
    c = Case(7, 5, lda=12, oa=1)
    op = _Quantize(c)
    op.fill(np.random.default_rng(24))
    with H.MMult(0, "auto") as own:
        side = _side_stream()
        mark = torch.zeros(4, device="cuda")
        seen = []

        def body():
            mark.fill_(1.0)   # (so that the graph is not empty)
            seen.append(_captured_nodes(side))
            with pytest.raises(H.MMultError) as e:
                op.call(own)
            seen.append(_captured_nodes(side))
            seen.append(e.value.status)
            del e   # (see _capture)

        graph = _capture(side, body)
        assert seen[2] == H.ERR_UNSUPPORTED and seen[1] == seen[0]
        graph.replay()
        torch.cuda.synchronize()
        assert bool((mark == 1.0).all()) and own.get_option(H.OPT_RETIRED_BUFFERS) == 0
        run_quantize(own, c, np.random.default_rng(25))   # uncaptured, the same call allocates and is exact
        del graph


# ---- a graph survives later growth ------------------------------------------------------------------------------------------
def _survives_growth(small, large, buffers, seed):
    """Capture `small`; `large`, eager, grows `buffers` of the images under the graph -- each must be retired, which the counter
    shows BEFORE the graph is replayed; then two replays on new inputs."""
    import how_to_optimize_gemm_amd as H
    assert grown(small, large) == buffers
    rng = np.random.default_rng(seed)
    with H.MMult(0, "auto") as own:
        side = _side_stream()
        _eager(own, side, [small], rng)
        graph = _capture(side, lambda: small.call(own))
        before = own.get_option(H.OPT_RETIRED_BUFFERS)
        assert before == 0
        _eager(own, side, [large], rng, "eager growth under a graph")
        assert own.get_option(H.OPT_RETIRED_BUFFERS) - before == buffers   # (a build that frees instead stops here)
        _replays(graph, [small], rng, 2)
        _eager(own, side, [large], rng, "the grown scratch beside the graph")
        assert own.get_option(H.OPT_RETIRED_BUFFERS) - before == buffers
        del graph


def test_a_graph_survives_a_fused_qgemm_that_grows_the_scratch():
    _survives_growth(_Qgemm(THIN_K), _Qgemm(RAGGED), 2, 31)


def test_a_graph_survives_a_two_pass_qgemm_that_grows_the_scratch():
    _survives_growth(_Qgemm(THIN_K, mode=5), _Qgemm(MID, mode=5), 3, 32)


def test_a_graph_survives_an_igemm_copy_that_grows_the_scratch():
    _survives_growth(_Igemm(MISALIGNED[0]), _Igemm(MISALIGNED_LARGE), 2, 33)


def test_an_eager_only_handle_retires_nothing():
    """The same sizes without a capture: growth frees, as before."""
    import how_to_optimize_gemm_amd as H
    rng = np.random.default_rng(34)
    with H.MMult(0, "auto") as own:
        side = _side_stream()
        for op in (_Qgemm(THIN_K), _Qgemm(RAGGED), _Qgemm(THIN_K, mode=5), _Qgemm(MID, mode=5), _Igemm(MISALIGNED[0]),
                   _Igemm(MISALIGNED_LARGE)):
            _eager(own, side, [op], rng)
        assert own.get_option(H.OPT_RETIRED_BUFFERS) == 0


# ---- two handles, two streams -----------------------------------------------------------------------------------------------
def test_two_handles_on_two_streams_overlap():
    """One handle per stream, as the header tells callers whose quantised calls should overlap: four calls each, issued in
    turn with no synchronisation in between."""
    import torch
    import how_to_optimize_gemm_amd as H
    rng = np.random.default_rng(41)
    cases = (RAGGED, COLUMN, MID, THIN_K)
    with H.MMult(0, "auto") as one, H.MMult(0, "auto") as two:
        handles, streams = (one, two), (torch.cuda.Stream(), torch.cuda.Stream())
        ops = [[_Qgemm(c) for c in cases], [_Qgemm(c) for c in reversed(cases)]]
        for op in ops[0] + ops[1]:
            op.fill(rng)
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
        for i in range(len(cases)):
            for h, s, mine in zip(handles, streams, ops):
                with torch.cuda.stream(s):
                    mine[i].call(h)
        torch.cuda.synchronize()
        for which, mine in enumerate(ops):
            for op in mine:
                op.check(f"handle {which}")


# ---- stale scratch never reaches a result -------------------------------------------------------------------------------------
def test_bytes_left_in_the_images_by_a_saturating_qgemm_reach_no_later_result():
    """After a call whose images are +-127 in every byte, the ragged shapes -- whose padded images (ka = (k + 15) & ~15,
    nb = (n + 3) & ~3) the quantiser writes k / n columns of -- are exact."""
    import how_to_optimize_gemm_amd as H
    cus = _cus()
    rng = np.random.default_rng(51)
    s = _big_side(cus)
    with H.MMult(0, "auto") as own:
        _eager(own, _side_stream(), [_Qgemm(Case(s, s, 272), saturate=True)], rng, "saturating")
        for c in (RAGGED, COLUMN, THIN_K):
            run_qgemm(own, 0, c, rng, cus)
        for c in (RAGGED, THIN_K):
            run_qgemm(own, 5, c, rng, cus)


def test_bytes_left_in_the_images_by_an_all_minus_128_copy_reach_no_later_result():
    import how_to_optimize_gemm_amd as H
    cus = _cus()
    rng = np.random.default_rng(52)
    with H.MMult(0, "auto") as own:
        _eager(own, _side_stream(), [_Igemm(MISALIGNED_LARGE, fill_value=-128)], rng, "all -128")
        for c in MISALIGNED:
            for accumulate in (False, True):
                run_igemm(own, 0, c, rng, cus, accumulate)


def test_growing_shrinking_and_growing_again_on_one_handle_is_exact_at_every_step():
    """Markers and bits at every step of a sequence that grows, shrinks and grows each image again, through all three users
    of qa / qb (fused, two-pass, copy); an eager-only handle: nothing is retired."""
    import how_to_optimize_gemm_amd as H
    cus = _cus()
    rng = np.random.default_rng(53)
    with H.MMult(0, "auto") as own:
        for entry, mode, c in (("qgemm", 0, THIN_K), ("qgemm", 0, RAGGED), ("igemm", 0, MISALIGNED[0]), ("qgemm", 5, MID),
                               ("qgemm", 0, THIN_K), ("igemm", 0, MISALIGNED_LARGE), ("qgemm", 5, Case(1, 1, 1)),
                               ("qgemm", 0, Case(1283, 1027, 129, lda=132, ldb=1028)), ("qgemm", 5, RAGGED), ("qgemm", 0, COLUMN),
                               ("igemm", 0, MISALIGNED[2]), ("qgemm", 0, RAGGED)):
            if entry == "qgemm":
                run_qgemm(own, mode, c, rng, cus)
            else:
                run_igemm(own, mode, c, rng, cus, False)
                run_igemm(own, mode, c, rng, cus, True)
        run_quantize(own, Case(301, 4097, lda=4100), rng)
        assert own.get_option(H.OPT_RETIRED_BUFFERS) == 0
