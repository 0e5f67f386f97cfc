"""The rows of tests/test_gpu_cold_start.py and the code that runs one: shared by the child processes, which run them on a handle
created with MMH_LAZY=1 (nothing opted into, queried or allocated before the first launch), and by the parent, which runs
them on a warmed handle and holds both to the oracle.  A row's inputs depend on its shapes and seed alone, so that two
processes draw the same numbers.  (Shared test code: see tests/bitcmp.py.)"""
import dataclasses
import functools
import hashlib
import math
import re

import numpy as np

import ex_ref
import relu_grad_ref
import splitk_ref
from kernel_tables import K2W_SK, OP_SHAPES, REG_TILES, _edge_cases, _edge_shapes, _streamk_shapes, _whole_shapes, per_cu_by_lds

# forced ids with a persistent stream-K form of their own (launch_reg.hip try_launch_streamk, launch_dma.hip, launch_dma5.hip)
STREAMK_KERNELS = ("mfma", "mfma_128x64", "mfma_256x256", "mfma_64x64", "mfma_64x64_dma", "mfma_128x64_dma", "mfma_128x128_dma",
                   "mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5")
SPLITK_KERNELS = ("mfma_splitk", "mfma_splitk_128x64")
# ids that launch another id's symbols at every shape here (K1 picks one of the valu_* tiles; mfma_tiles is mfma's plain launch):
# they run last, so that every other id's rows come first in the process
ALIASES = ("valu", "mfma_tiles")
assert len(K2W_SK) == 3 == sum(k.endswith("_dma5") for k in STREAMK_KERNELS)


def draw(seed, *shapes):
    """fp32 arrays uniform in [-1, 1) from numpy.random.default_rng(seed), in the order of `shapes`."""
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, s).astype(np.float32) for s in shapes]


def digest(*arrays):
    h = hashlib.sha256()
    for x in arrays:
        h.update(np.ascontiguousarray(x, dtype=np.float32).tobytes())
    return h.hexdigest()


def seed_of(*numbers):
    return int(hashlib.sha256(repr(numbers).encode()).hexdigest()[:8], 16)


# ---- child A: forced kernels through mmh_sgemm ----------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Forced:
    kernel: str
    form: str          # "whole", "guarded", "streamk", "streamk guarded", "streamk rounds", "splitk"
    m: int
    n: int
    k: int
    streamk: int = 1   # MMH_OPT_STREAMK (1: the handle's default)
    splitk: int = 0    # MMH_OPT_SPLITK

    @property
    def name(self):
        return f"{self.kernel} {self.form} {self.m}x{self.n}x{self.k}"


def tile_of(kernel):
    """BM, BN, KB of a forced id's tile (ids without one: the 128x128 tile of K2's rungs, one 64x64 block for K0 and K1)."""
    t = re.search(r"(\d+)x(\d+)", kernel)
    if kernel in REG_TILES:
        return REG_TILES[kernel][:2] + (REG_TILES[kernel][4],)
    if t:
        return int(t[1]), int(t[2]), 32
    return (64, 64, 32) if kernel in ("valu", "naive") else (128, 128, 32)


def lds_allows(kernel):
    """Persistent workgroups per CU the LDS allows a stream-K id: two K-slices (register-staged) or a ring of three."""
    bm, bn, kb = tile_of(kernel)
    return per_cu_by_lds(bm, bn, kb) if kernel in REG_TILES else (160 * 1024) // (3 * 32 * (bm + bn) * 4)


def forced_rows(cus, chain_kernels):
    """Per id the smallest shapes of the parity tables' generators that reach each launch form.  One whole tile (the plain
    launch's own opt-in) and one guarded shape; for ids with a stream-K form the first whole and the first guarded shape of
    _streamk_shapes -- (isqrt(CUs) + 1)^2 tiles: the fewest that hand over, the first launch that allocates the null stream's
    set, queries residency and asks for its LDS share -- and, where the LDS allows more than one workgroup per CU, the
    generator's second whole shape: more than two tiles per CU, the smallest count at which the GRID depends on the
    residency the launch has just queried (the first shapes fill one workgroup per CU whatever it says).

    ORDER.  Every row is the first launch of its kernel symbol in the child: ids in catalogue order, a whole-tile shape and a
    guarded one are two instantiations, the stream-K forms two more, and no id falls back to another's tile at these shapes --
    except the rows that have no symbol of their own: ALIASES, which run last, and valu_128x64's guarded row (K1W has whole
    tiles only: it runs K1's guarded 128x128 tile, as valu_128x128's does)."""
    own = [k for k in chain_kernels if k != "auto" and k not in ALIASES]
    rows = []
    for kernel in own + [k for k in ALIASES if k in chain_kernels]:
        bm, bn, kb = tile_of(kernel)
        whole = _edge_cases(bm, bn, kb)[-1] if kb != 32 else None
        whole = (whole.m, whole.n, whole.k) if whole else _whole_shapes(bm, bn)[0]
        assert whole == (bm, bn, kb), (kernel, whole)
        guarded = _edge_shapes(bm, bn)[2]
        assert guarded == (bm + 1, 2 * bn - 1, 33), (kernel, guarded)
        rows += [Forced(kernel, "whole", *whole), Forced(kernel, "guarded", *guarded)]
        if kernel in STREAMK_KERNELS:
            rows.append(Forced(kernel, "streamk", *_streamk_shapes(bm, bn, False, False)(cus)[0][:3], streamk=2))
            rows.append(Forced(kernel, "streamk guarded", *_streamk_shapes(bm, bn, True, False)(cus)[0][:3], streamk=2))
            if lds_allows(kernel) > 1:
                rows.append(Forced(kernel, "streamk rounds", *_streamk_shapes(bm, bn, False, False)(cus)[1][:3], streamk=2))
    # tests/test_gpu_splitk_parity.py's smallest case: one tile, two K-slices, two parts asked for
    rows += [Forced(kernel, "splitk", *tile_of(kernel)[:2], 64, splitk=2) for kernel in SPLITK_KERNELS]
    assert len({r.name for r in rows}) == len(rows)
    return rows


@functools.lru_cache(maxsize=None)
def forced_inputs(m, n, k):
    return tuple(draw(seed_of("forced", m, n, k), (m, k), (k, n)))


def run_forced(mm, row, stream=0):
    """The row through mmh_sgemm on dense operands, C NaN beforehand: (launch string, C)."""
    import torch
    import how_to_optimize_gemm_amd as H
    a, b = forced_inputs(row.m, row.n, row.k)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    c = torch.full((row.m, row.n), float("nan"), device="cuda")
    torch.cuda.synchronize()
    mm.set_kernel(row.kernel)
    mm.set_streamk(row.streamk)
    mm.set_splitk(row.splitk)
    try:
        mm.sgemm(row.m, row.n, row.k, da.data_ptr(), row.k, db.data_ptr(), row.n, c.data_ptr(), row.n, False, stream)
        launched = H.last_launch()
        torch.cuda.synchronize()
    finally:
        mm.set_streamk(1)
        mm.set_splitk(0)
    return launched, c.cpu().numpy()


def check_forced_launch(row, launched):
    """The launch string says the row reached its form."""
    at = (row.name, launched)
    bm, bn, _ = tile_of(row.kernel)
    if row.form == "splitk":
        assert f"sgemm_mfma_splitk_kernel<{bm},{bn}>" in launched and "1 tiles x 2 concurrent K parts" in launched, at
        return
    sk = re.search(r"(\d+) tiles on (\d+) persistent", launched)
    if row.form.startswith("streamk"):
        assert sk and "streamk_kernel" in launched, at
        tiles, grid = int(sk[1]), int(sk[2])
        assert tiles == -(-row.m // bm) * -(-row.n // bn) and tiles > grid and tiles % grid != 0, at   # tiles are handed over
    else:
        assert sk is None and "streamk" not in launched and "splitk" not in launched, at
    if row.kernel != "naive":
        # (mfma_64x64's K-slices are 128 deep: the generator's k = 160 makes its whole-tile stream-K row a guarded launch too)
        assert ("guarded" in launched) == ("guarded" in row.form or row.k % tile_of(row.kernel)[2] != 0), at
        if row.kernel not in ALIASES and row.name != f"valu_128x64 guarded {bm + 1}x{2 * bn - 1}x33":
            assert f"<{bm},{bn}>" in launched, at


@functools.lru_cache(maxsize=None)
def forced_reference(row):
    from oracle import oracle as O
    a, b = forced_inputs(row.m, row.n, row.k)
    if row.form == "splitk":
        return splitk_ref.splitk_ref(O, a, b, None, row.splitk)
    return O.ref_mmult(a, b, fma=True)


# ---- child B: MMH_KERNEL_AUTO through the tensor front ends -----------------------------------------------------------------
# Each step: (name, run(mm, cus) -> (launch string, [results as numpy]), reference(cus) -> [expected], planned(cus) -> the grid,
# part or workgroup count of the host plan, which the launch string must carry).  Shapes are the parity modules' own or smaller: OP_SHAPES
# (tests/test_gpu_op.py, test_gpu_ex.py), tests/test_batched_plan.py's fold and one-launch examples, test_gpu_splitk_parity.py's
# "chosen part count, AUTO".
OP_SHAPE = OP_SHAPES[1]        # (512, 384, 1024): NT / TN / TT, linear, addmm
assert OP_SHAPE == (512, 384, 1024)
BMM_ONE = (128, 128, 128, 16)  # m, n, k, batch
BMM_FOLD = (256, 256, 256, 8)  # B shared by the batch (stride 0)
BLINEAR = (128, 128, 128, 4)   # rows, out, in, batch
BACKWARD = (512, 384, 256)     # rows, out, in
SPLIT_AUTO = (128, 128, 512)   # one 128x128 tile: MMH_OPT_SPLITK = 1 splits it


def matmul_shape(cus, streamk):
    """The first OP_SHAPES entry up to 2176^3 that MMH_KERNEL_AUTO plans as a stream-K launch (grid > 0) / a plain one (0)."""
    import how_to_optimize_gemm_amd as H
    for shape in OP_SHAPES:
        if max(shape) <= 2176 and (H.auto_plan(*shape, cu_count=cus)[2] > 0) == streamk:
            return shape
    raise AssertionError(("no OP_SHAPES entry with such a plan", cus, streamk))


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _launched(run):
    """run() on the current stream; (launch string, results on the host)."""
    import torch
    import how_to_optimize_gemm_amd as H
    out = run()
    launched = H.last_launch()
    torch.cuda.synchronize()
    return launched, [t.cpu().numpy() for t in (out if isinstance(out, (tuple, list)) else [out])]


def _chain(a, b):
    from oracle import oracle as O
    return O.ref_mmult(np.ascontiguousarray(a), np.ascontiguousarray(b), fma=True)


@functools.lru_cache(maxsize=None)
def _gemm_inputs(tag, m, n, k):
    return tuple(draw(seed_of(tag, m, n, k), (m, k), (k, n), (m, n), (n,)))   # A, B, C, a column bias


@functools.lru_cache(maxsize=None)
def _batch_inputs(tag, m, n, k, batch, shared_b):
    return tuple(draw(seed_of(tag, m, n, k, batch), (batch, m, k), (1 if shared_b else batch, k, n), (batch, n)))


@functools.lru_cache(maxsize=None)
def _backward_inputs():
    rows, n_out, n_in = BACKWARD
    return tuple(draw(seed_of("backward", *BACKWARD), (rows, n_out), (rows, n_in), (n_out, n_in), (rows, n_out)))   # g, x, w, y


def _matmul_step(streamk):
    def run(mm, cus):
        a, b, _, _ = _gemm_inputs("matmul", *matmul_shape(cus, streamk))
        return _launched(lambda: mm.matmul(_dev(a), _dev(b)))

    def reference(cus):
        a, b, _, _ = _gemm_inputs("matmul", *matmul_shape(cus, streamk))
        return [_chain(a, b)]

    def planned(cus):
        import how_to_optimize_gemm_amd as H
        _, tiles, grid = H.auto_plan(*matmul_shape(cus, streamk), cu_count=cus)
        return grid if streamk else tiles
    return ("matmul, a stream-K plan" if streamk else "matmul, a plain plan"), run, reference, planned


def _op_step(ta, tb):
    m, n, k = OP_SHAPE

    def run(mm, cus):
        a, b, _, _ = _gemm_inputs("op", m, n, k)
        da, db = (_dev(a.T).t() if ta else _dev(a)), (_dev(b.T).t() if tb else _dev(b))   # transposed views, read in place
        return _launched(lambda: mm.matmul(da, db))

    def planned(cus):
        import how_to_optimize_gemm_amd as H
        return H.auto_plan_op(ta, tb, m, n, k, cu_count=cus)[1]
    return "sgemm_op " + "NT"[ta] + "NT"[tb], run, lambda cus: [_chain(*_gemm_inputs("op", m, n, k)[:2])], planned


def _linear_step():
    m, n, k = OP_SHAPE

    def run(mm, cus):
        x, w, _, bias = _gemm_inputs("linear", m, n, k)
        return _launched(lambda: mm.linear(_dev(x), _dev(w.T), _dev(bias), "relu"))   # w stored out x in

    def reference(cus):
        x, w, _, bias = _gemm_inputs("linear", m, n, k)
        return [ex_ref.expected(_chain(x, w), 1.0, 0.0, None, bias, ex_ref.COL, ex_ref.RELU)]

    def planned(cus):
        import how_to_optimize_gemm_amd as H
        return H.auto_plan_ex(0, 1, m, n, k, cu_count=cus)[1]
    return "linear, bias and ReLU", run, reference, planned


ADDMM_ALPHA, ADDMM_BETA = 1.5, -0.75


def _addmm_step():
    m, n, k = OP_SHAPE

    def run(mm, cus):
        a, b, c, _ = _gemm_inputs("addmm", m, n, k)
        return _launched(lambda: mm.addmm(_dev(c), _dev(a), _dev(b), beta=ADDMM_BETA, alpha=ADDMM_ALPHA))

    def reference(cus):
        a, b, c, _ = _gemm_inputs("addmm", m, n, k)
        return [ex_ref.expected(_chain(a, b), ADDMM_ALPHA, ADDMM_BETA, c, None, ex_ref.NONE, 0)]

    def planned(cus):
        import how_to_optimize_gemm_amd as H
        return H.auto_plan_ex(0, 0, m, n, k, cu_count=cus)[1]
    return "addmm, beta != 0", run, reference, planned


def _bmm_step(shape, form):
    m, n, k, batch = shape
    shared = form == "fold"

    def plan(cus):
        import how_to_optimize_gemm_amd as H
        kern, got, wgs = H.auto_plan_batched(0, 0, m, n, k, batch=batch, stride_b=0 if shared else -1, cu_count=cus)
        assert got == form, (shape, form, got)
        return wgs

    def run(mm, cus):
        plan(cus)
        a, b, _ = _batch_inputs("bmm", m, n, k, batch, shared)
        db = _dev(b[0]).unsqueeze(0).expand(batch, -1, -1) if shared else _dev(b)
        return _launched(lambda: mm.bmm(_dev(a), db))

    def reference(cus):
        a, b, _ = _batch_inputs("bmm", m, n, k, batch, shared)
        return [np.stack([_chain(a[i], b[0 if shared else i]) for i in range(batch)])]
    return f"bmm, {form}", run, reference, plan


def _batched_linear_step():
    rows, n_out, n_in, batch = BLINEAR

    def run(mm, cus):
        x, wt, bias = _batch_inputs("blinear", rows, n_out, n_in, batch, False)   # wt[i]: in x out
        w = _dev(np.ascontiguousarray(wt.transpose(0, 2, 1)))                     # stored out x in, read in place
        return _launched(lambda: mm.batched_linear(_dev(x), w, _dev(bias), "relu"))

    def reference(cus):
        x, wt, bias = _batch_inputs("blinear", rows, n_out, n_in, batch, False)
        return [np.stack([ex_ref.expected(_chain(x[i], wt[i]), 1.0, 0.0, None, bias[i], ex_ref.COL, ex_ref.RELU) for i in range(batch)])]

    def planned(cus):
        import how_to_optimize_gemm_amd as H
        return H.auto_plan_batched_ex(0, 1, rows, n_out, n_in, stride_bias=n_out, bias_mode=H.BIAS_COL, batch=batch, cu_count=cus)[2]
    return "batched_linear, a bias per matrix", run, reference, planned


def _backward_step():
    def run(mm, cus):
        g, x, w, y = _backward_inputs()
        return _launched(lambda: mm.linear_backward(_dev(g), _dev(x), _dev(w), _dev(y)))   # (dx, dw, db); the last launch is dw's TN

    def reference(cus):
        import how_to_optimize_gemm_amd as H
        g, x, w, y = _backward_inputs()
        dz, db = relu_grad_ref.relu_grad_colsum(g, y, H.COLSUM_BLOCK_ROWS)
        return [_chain(dz, w), _chain(dz.T, x), db]

    def planned(cus):
        import how_to_optimize_gemm_amd as H
        rows, n_out, n_in = BACKWARD
        return H.auto_plan_op(1, 0, n_out, n_in, rows, cu_count=cus)[1]
    return "linear_backward with y", run, reference, planned


def _split_step():
    m, n, k = SPLIT_AUTO

    def parts(cus):
        return splitk_ref.parts_launched(splitk_ref.auto_parts(cus, 1, k), k // 32)

    def run(mm, cus):
        a, b, _, _ = _gemm_inputs("split", m, n, k)
        mm.set_splitk(1)
        try:
            return _launched(lambda: mm.matmul(_dev(a), _dev(b)))
        finally:
            mm.set_splitk(0)

    def reference(cus):
        from oracle import oracle as O
        a, b, _, _ = _gemm_inputs("split", m, n, k)
        return [splitk_ref.splitk_ref(O, a, b, None, parts(cus))]
    return "matmul that splits", run, reference, parts


def auto_steps():
    """Each step is the first use of its form in the child: the NN stream-K and plain launches, the three op forms, the `ex`
    NT and NN forms, the batched and batched `ex` forms, mmh_relu_grad_colsum, and the opt-in split-K."""
    return [_matmul_step(True), _matmul_step(False), _op_step(0, 1), _op_step(1, 0), _op_step(1, 1), _linear_step(), _addmm_step(),
            _bmm_step(BMM_ONE, "one_launch"), _bmm_step(BMM_FOLD, "fold"), _batched_linear_step(), _backward_step(), _split_step()]


def carried_count(name, launched):
    """The number a launch string carries where the plan functions return one: the persistent grid, the concurrent K parts,
    or the workgroups -- parsed as tests/test_gpu_round3.py::test_the_host_plan_is_what_the_device_launches does."""
    sk = re.search(r"(\d+) tiles on (\d+) persistent", launched)
    if sk:
        return int(sk[2])
    parts = re.search(r"(\d+) tiles x (\d+) concurrent K parts", launched)
    if parts:
        return int(parts[2])
    wgs = re.search(r"(\d+) workgroups", launched)
    assert wgs, (name, launched)
    return int(wgs[1])


# ---- child C: capture -------------------------------------------------------------------------------------------------------
def capture_rows(cus):
    r = math.isqrt(cus) + 1
    rows = [Forced("mfma_128x128_dma5", "whole", 128, 128, 32),                      # a 96 KiB opt-in inside the capture
            Forced("mfma_128x64_dma5", "streamk", r * 128, r * 64, 160, streamk=2)]  # child A's stream-K shape
    assert rows[1] in forced_rows(cus, ["mfma_128x64_dma5"]) and rows[0] in forced_rows(cus, ["mfma_128x128_dma5"])
    return rows


# ---- the children -----------------------------------------------------------------------------------------------------------
def _cold_handle():
    """A handle that has skipped the warm-up, in a process that has launched nothing."""
    import how_to_optimize_gemm_amd as H
    assert H.last_launch() == "", H.last_launch()
    mm = H.MMult(0, "auto")
    assert mm.get_option(H.OPT_WARMED) == 0, "MMH_LAZY=1 did not keep mmh_create from warming the handle"
    assert H.last_launch() == "", H.last_launch()
    return mm, mm.device_info()["cu_count"]


def child_forced():
    import how_to_optimize_gemm_amd as H
    mm, cus = _cold_handle()
    out = {"cus": cus, "rows": {}}
    for row in forced_rows(cus, H.CHAIN_KERNELS):
        launched, got = run_forced(mm, row)
        assert mm.streamk_timeouts() == 0, row.name
        out["rows"][row.name] = {"launch": launched, "sha256": digest(got)}
    assert mm.get_option(H.OPT_WARMED) == 0
    mm.close()
    return out


def child_auto():
    import os
    import how_to_optimize_gemm_amd as H
    mm, cus = _cold_handle()
    out = {"cus": cus, "rows": {}}
    steps = auto_steps()
    for name, run, _, _ in steps:
        launched, got = run(mm, cus)
        assert mm.streamk_timeouts() == 0, name
        out["rows"][name] = {"launch": launched, "sha256": digest(*got)}
    # warming afterwards changes nothing: the first step again, the same launch and the same bits
    assert mm.get_option(H.OPT_WARMED) == 0
    mm.warm()
    assert mm.get_option(H.OPT_WARMED) == 1
    mm.warm()
    assert mm.get_option(H.OPT_WARMED) == 1
    name, run, _, _ = steps[0]
    launched, got = run(mm, cus)
    assert mm.streamk_timeouts() == 0
    out["repeat"] = {"launch": launched, "sha256": digest(*got)}
    # a warmed handle beside the lazy one: the per-handle residency cache and the process-wide opt-in list, whichever came first
    del os.environ["MMH_LAZY"]
    warmed = H.MMult(0, "auto")
    assert warmed.get_option(H.OPT_WARMED) == 1
    out["beside"] = {}
    for row in forced_rows(cus, ["mfma_128x64_dma5"]):
        if not row.form.startswith("streamk"):
            continue
        for who, h in (("created warmed", warmed), ("created lazy", mm)):
            launched, got = run_forced(h, row)
            assert h.streamk_timeouts() == 0, (row.name, who)
            out["beside"][f"{row.name}, {who}"] = {"launch": launched, "sha256": digest(got)}
    warmed.close()
    mm.close()
    return out


def child_capture():
    import torch
    import how_to_optimize_gemm_amd as H
    mm, cus = _cold_handle()
    out = {"cus": cus, "rows": {}}
    side = torch.cuda.Stream()
    for row in capture_rows(cus):
        a, b = forced_inputs(row.m, row.n, row.k)
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        c = torch.full((row.m, row.n), float("nan"), device="cuda")
        torch.cuda.synchronize()
        side.wait_stream(torch.cuda.current_stream())
        mm.reserve_stream(side.cuda_stream, row.m, row.n, row.k)
        mm.set_kernel(row.kernel)
        mm.set_streamk(row.streamk)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                mm.matmul(da, db, out=c)           # the kernel's first launch in the process, on a capturing stream
                captured = H.last_launch()
        torch.cuda.current_stream().wait_stream(side)
        results = []
        for _ in range(2):
            c.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            results.append(c.cpu().numpy())
        c.fill_(float("nan"))
        mm.matmul(da, db, out=c)
        eager = H.last_launch()
        torch.cuda.synchronize()
        results.append(c.cpu().numpy())
        mm.set_streamk(1)
        assert not np.isnan(results[0]).any(), (row.name, "the replay left NaN in C")
        assert digest(results[0]) == digest(results[1]) == digest(results[2]), (row.name, "replays and the eager call differ")
        assert mm.streamk_timeouts() == 0, row.name
        out["rows"][row.name] = {"launch": eager, "captured": captured, "sha256": digest(results[2])}
    assert mm.get_option(H.OPT_RETIRED_BUFFERS) == 0
    mm.close()
    return out
