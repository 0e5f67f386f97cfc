"""Python host side over the C ABI of libmmult_hip.so (include/mmult_hip.h).

Mirrors the reference's operator interface for the hot path -- the names,
argument order and semantics of `MY_MMult(m, n, k, a, lda, b, ldb, c, ldc)`
(host flavour: armv7/test_MMult.c:8,76 / aarch64/test_MMult.cpp:17,113,
C += A*B on host buffers; device flavour: cuda/test_MMult.cpp:13-14,102,
C = A*B on device pointers, asynchronous) -- so parity tests read like the
reference's own harness.  PyTorch appears only as a source of device memory,
streams and torch.distributed; every FLOP is issued by the HIP library.

There is NO CPU fallback: if the library or a gfx950 device is missing, calls
raise MMultError.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import abi_header as _abi

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libmmult_hip.so")
AB_LIB_PATH = os.path.join(PKG_DIR, "libmmult_hip_ab.so")   # tools-only build (see use_ab_library)

# Every MMH_* constant and every prototype comes from include/mmult_hip.h itself (abi_header.py).  These are module names here,
# the header's values under the header's names less the MMH_ prefix: OK, ERR_COMM, KERNEL_AUTO, OPT_STREAMK, OP_T, BIAS_ROW, ...
_CONSTANT_PREFIXES = ("OK", "ERR_", "KERNEL_", "OPT_", "OP_", "BIAS_", "ACT_", "BATCHED_MAX_WORKGROUPS", "COLSUM_BLOCK_ROWS")
_CONSTANTS = {name: v for name, v in _abi.constants("MMH_").items() if name.startswith(_CONSTANT_PREFIXES)}
globals().update(_CONSTANTS)
BATCH_FORMS = {v: name.lower() for name, v in _abi.constants("MMH_BATCH_FORM_").items()}   # mmh_sgemm_batched's forms, by value
# short name -> id: the header's MMH_KERNEL_ names in lower case ("mfma256" is the library's own short name of MMH_KERNEL_MFMA_256)
KERNELS = {{"mfma_256": "mfma256"}.get(name.lower(), name.lower()): v for name, v in _abi.constants("MMH_KERNEL_").items()}
# (tools build only, libmmult_hip_ab.so: the 32x32x2 tiles mfma32_* / mfma32b_* (ids 48-51, 60-62), exp5_*, the rim --
# their names resolve through the library's own table, mmh_kernel_id)
# kernels that keep the one-chain-per-element contract (bit-identical results); the split-K ids do not
CHAIN_KERNELS = [k for k in KERNELS if "splitk" not in k]
_SHORT_NAMES = {v: name for name, v in KERNELS.items() if name != "mfma256"}   # what the plan functions (auto_plan*) call a kernel id

EXPORTS = list(_abi.PROTOTYPES)   # every symbol include/mmult_hip.h declares (tests assert the .so exports them all)


class MMultError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where}: status {status} ({detail})")


_lib: Optional[C.CDLL] = None
_lib_path = LIB_PATH


def use_ab_library(build: bool = True) -> str:
    """tools/ only: load libmmult_hip_ab.so (the product kernels plus the scheduling A/B variants, the families that
    measured slower -- the 32x32x2 tiles, the rim -- and the timing-only ablation builds, whose results are WRONG)
    instead of the product library.  Must be called before the first lib(); builds the library on demand
    (build=False: only if it is already there -- raises otherwise)."""
    global _lib_path
    if _lib is not None and _lib_path != AB_LIB_PATH:
        raise MMultError(ERR_INVALID_ARG, "use_ab_library", "the product library is already loaded")
    if build:
        from . import build as _build
        _build.build_ab_library()
    elif not os.path.exists(AB_LIB_PATH):
        raise MMultError(ERR_UNSUPPORTED, "use_ab_library", "libmmult_hip_ab.so has not been built")
    _lib_path = AB_LIB_PATH
    return AB_LIB_PATH


def streamk_plan(tiles: int, nk: int, grid: int):
    """(order, place) of a phase-ordered stream-K launch as numpy int32 arrays (host arithmetic only)."""
    order = np.zeros(grid, dtype=np.int32)
    place = np.zeros(tiles, dtype=np.int32)
    _check(lib().mmh_streamk_plan(tiles, nk, grid, order.ctypes.data_as(C.POINTER(C.c_int)),
                                  place.ctypes.data_as(C.POINTER(C.c_int))), "mmh_streamk_plan")
    return order, place


def _dense_ld(transa, transb, m, n, k, lda, ldb, ldc):   # the plan functions' (lda, ldb, ldc): 0 = the dense stored row (k or m, n or k, n)
    return lda or (m if transa else k), ldb or (k if transb else n), ldc or n


def auto_plan(m: int, n: int, k: int, lda: int = 0, ldb: int = 0, ldc: int = 0, base_align: int = 16, cu_count: int = 256):
    """What MMH_KERNEL_AUTO would run for a shape (host arithmetic only, no device): (short kernel name, tiles,
    stream-K grid) -- grid 0 = one workgroup per tile, -1 = needs the device's occupancy query."""
    kern, grid, tiles = C.c_int(), C.c_int(), C.c_long()
    _check(lib().mmh_auto_plan(m, n, k, *_dense_ld(OP_N, OP_N, m, n, k, lda, ldb, ldc), base_align, cu_count, C.byref(kern),
                               C.byref(tiles), C.byref(grid)), "mmh_auto_plan")
    return _SHORT_NAMES.get(kern.value, str(kern.value)), tiles.value, grid.value


def igemm_plan(entry: str, mode: int, m: int, n: int, k: int, lda: int = 0, ldb: int = 0, ldc: int = 0, a_mod16: int = 0,
               b_mod16: int = 0, c_mod16: int = 0, cu_count: int = 256, grid_cap: int = 0):
    """What MMult.igemm_s8 (entry "igemm") or MMult.qgemm ("qgemm") would do in MMH_OPT_IGEMM_MODE `mode` (host arithmetic only,
    no device): (what last_launch() says after the call, {"qa", "qb", "qc", "qs", "bt": bytes of the handle's scratch the call
    needs}).  x_mod16: the operands' base addresses modulo 16; grid_cap: the MMH_I8_GRID_CAP test hook.  Raises for a mode this
    build does not accept, as set_igemm_mode does."""
    text, sizes = C.create_string_buffer(256), (C.c_size_t * 5)()
    _check(lib().mmh_igemm_plan(_abi.constants("MMH_I8_")[entry.upper()], mode, m, n, k, lda or k, ldb or n, ldc or n, a_mod16, b_mod16, c_mod16,
                                cu_count, grid_cap, text, len(text), sizes), "mmh_igemm_plan")
    return text.value.decode(), dict(zip(("qa", "qb", "qc", "qs", "bt"), sizes))


def _plan_op(name, transa, transb, m, n, k, lda, ldb, ldc, base_align, cu_count):
    """auto_plan_op / auto_plan_ex: mmh_auto_plan_op's arguments and result triple."""
    kern, grid, tiles = C.c_int(), C.c_int(), C.c_long()
    _check(getattr(lib(), name)(transa, transb, m, n, k, *_dense_ld(transa, transb, m, n, k, lda, ldb, ldc), base_align, cu_count,
                                C.byref(kern), C.byref(tiles), C.byref(grid)), name)
    return _SHORT_NAMES.get(kern.value, str(kern.value)), tiles.value, grid.value


def auto_plan_op(transa: int, transb: int, m: int, n: int, k: int, lda: int = 0, ldb: int = 0, ldc: int = 0, base_align: int = 16,
                 cu_count: int = 256):
    """auto_plan for mmh_sgemm_op (OP_N / OP_T per operand; lda / ldb default to the dense stored rows: k or m, n or k)."""
    return _plan_op("mmh_auto_plan_op", transa, transb, m, n, k, lda, ldb, ldc, base_align, cu_count)


def auto_plan_ex(transa: int, transb: int, m: int, n: int, k: int, lda: int = 0, ldb: int = 0, ldc: int = 0, base_align: int = 16,
                 cu_count: int = 256):
    """auto_plan for mmh_sgemm_ex: planned like an op form -- one of the 64x64 / 128x64 / 128x128 LDS-DMA tiles -- for
    (OP_N, OP_N) too."""
    return _plan_op("mmh_auto_plan_ex", transa, transb, m, n, k, lda, ldb, ldc, base_align, cu_count)


def _plan_batched(name, transa, transb, m, n, k, lda, ldb, ldc, stride_a, stride_b, stride_c, *rest):
    """auto_plan_batched / auto_plan_batched_ex: the dense leading dimensions, the packed matrices a negative stride stands for,
    `rest` -- what the C function takes between strideC and its results -- and the result triple."""
    lda, ldb, ldc = _dense_ld(transa, transb, m, n, k, lda, ldb, ldc)
    sa = (k if transa else m) * lda if stride_a < 0 else stride_a
    sb = (n if transb else k) * ldb if stride_b < 0 else stride_b
    sc = m * ldc if stride_c < 0 else stride_c
    kern, form, wgs = C.c_int(), C.c_int(), C.c_long()
    _check(getattr(lib(), name)(transa, transb, m, n, k, lda, ldb, ldc, sa, sb, sc, *rest, C.byref(kern), C.byref(form),
                                C.byref(wgs)), name)
    return _SHORT_NAMES.get(kern.value, str(kern.value)), BATCH_FORMS.get(form.value, str(form.value)), wgs.value


def auto_plan_batched(transa: int, transb: int, m: int, n: int, k: int, lda: int = 0, ldb: int = 0, ldc: int = 0,
                      stride_a: int = -1, stride_b: int = -1, stride_c: int = -1, batch: int = 1, base_align: int = 16,
                      cu_count: int = 256):
    """What MMH_KERNEL_AUTO would run for mmh_sgemm_batched (host arithmetic only): (short kernel name, form name --
    "fold", "one_launch" or "loop" --, workgroups of all its launches).  Strides default to the packed matrices."""
    return _plan_batched("mmh_auto_plan_batched", transa, transb, m, n, k, lda, ldb, ldc, stride_a, stride_b, stride_c, batch,
                         base_align, cu_count)


def auto_plan_batched_ex(transa: int, transb: int, m: int, n: int, k: int, lda: int = 0, ldb: int = 0, ldc: int = 0,
                         stride_a: int = -1, stride_b: int = -1, stride_c: int = -1, stride_bias: int = 0,
                         bias_mode: int = BIAS_NONE, batch: int = 1, base_align: int = 16, cu_count: int = 256):
    """auto_plan_batched for mmh_sgemm_batched_ex: the fold form only where the biases fold too (no bias, a column bias with
    stride_bias == 0, a row bias with stride_bias == m), the loop form at batch x auto_plan_ex's per-matrix plan."""
    return _plan_batched("mmh_auto_plan_batched_ex", transa, transb, m, n, k, lda, ldb, ldc, stride_a, stride_b, stride_c,
                         stride_bias, int(bias_mode), batch, base_align, cu_count)


def use_timeline_library() -> str:
    """tools/dma_timeline.py only: the A/B library built with per-workgroup timeline stamps."""
    global _lib_path
    if _lib is not None:
        raise MMultError(ERR_INVALID_ARG, "use_timeline_library", "a library is already loaded")
    from . import build as _build
    _lib_path = _build.build_timeline_library()
    return _lib_path


def _share_hip_runtime_with_torch() -> None:
    """One process must hold ONE HIP runtime.  PyTorch's ROCm wheels bundle their
    own libamdhip64.so.7; libmmult_hip.so needs the same SONAME.  If this
    library pulled in /opt/rocm's copy first, a later `import torch` would load a
    second runtime and find "No HIP GPUs".  So when torch is installed (it need
    not be imported), its copy is loaded first and ours binds to it.  C/C++
    callers without torch in the process simply use /opt/rocm's runtime."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib() -> C.CDLL:
    """Load libmmult_hip.so (built in-tree by build.py).  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    _share_hip_runtime_with_torch()
    if not os.path.exists(_lib_path):
        raise MMultError(ERR_UNSUPPORTED, "load",
                         f"{_lib_path} is missing -- run __graft_entry__.build(); "
                         "there is no CPU fallback")
    L = C.CDLL(_lib_path)
    for name, (restype, argtypes) in _abi.PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _check(status: int, where: str) -> None:
    if status != OK:
        L = lib()
        detail = L.mmh_strerror(status).decode()
        last = L.mmh_last_error().decode()
        raise MMultError(status, where, f"{detail}; {last}" if last else detail)


def device_count() -> int:
    n = C.c_int(0)
    _check(lib().mmh_device_count(C.byref(n)), "mmh_device_count")
    return n.value


def rccl_version() -> int:
    """ncclGetVersion's code as libmmult_hip.so sees RCCL (dlopen); raises MMultError(ERR_UNSUPPORTED)
    when librccl or an entry point the shard needs is missing.  Needs no GPU."""
    v = C.c_int(0)
    _check(lib().mmh_rccl_version(C.byref(v)), "mmh_rccl_version")
    return v.value


def shard_chunks(k: int, b_chunks: int) -> list[int]:
    """K boundaries of mmh_shard_sgemm_streamed's broadcast chunks (host arithmetic, no GPU): [0, ..., k]."""
    k0 = (C.c_int * 65)()
    c = lib().mmh_shard_chunks(int(k), int(b_chunks), k0)
    if c < 0:
        raise MMultError(c, "mmh_shard_chunks")
    return [k0[i] for i in range(c + 1)]


def shard_rows(m: int, nranks: int, rank: int) -> tuple[int, int]:
    """(row0, rows) of the C/A row panel owned by `rank` (pure host arithmetic)."""
    r0, nr = C.c_int(0), C.c_int(0)
    _check(lib().mmh_shard_rows(m, nranks, rank, C.byref(r0), C.byref(nr)), "mmh_shard_rows")
    return r0.value, nr.value


def last_launch() -> str:
    """Which kernel configuration the last sgemm call on this thread launched."""
    return lib().mmh_last_launch().decode()


def kernel_name(kernel: int) -> Optional[str]:
    s = lib().mmh_kernel_name(kernel)
    return s.decode() if s else None


def _kernel_id(kernel) -> int:
    if isinstance(kernel, str):
        if kernel in KERNELS:
            return KERNELS[kernel]
        kid = lib().mmh_kernel_id(kernel.encode())      # the library's own table (A/B ids of the tools build too)
        if kid < 0:
            raise KeyError(kernel)
        return kid
    return int(kernel)


def _np_ptr(x: np.ndarray) -> int:
    return x.ctypes.data


class MMult:
    """One handle = one device + the selected kernel variant (the reference's
    cublasHandle_t lifetime, cuda/test_MMult.cpp:43-44,142)."""

    def __init__(self, device: int = 0, kernel="auto"):
        self._h = C.c_void_p(None)
        _check(lib().mmh_create(C.byref(self._h), device), "mmh_create")
        self.device = device
        self.set_kernel(kernel)

    def close(self) -> None:
        if self._h:
            lib().mmh_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def warm(self) -> None:
        """Everything a first launch would pay for (code objects, LDS opt-ins, residency queries, stream-K
        workspaces) -- mmh_create does it already unless MMH_LAZY=1; idempotent."""
        _check(lib().mmh_warm(self._h), "mmh_warm")

    # -- configuration ------------------------------------------------------
    def set_kernel(self, kernel) -> None:
        _check(lib().mmh_set_kernel(self._h, _kernel_id(kernel)), "mmh_set_kernel")

    def get_kernel(self) -> int:
        k = C.c_int(0)
        _check(lib().mmh_get_kernel(self._h, C.byref(k)), "mmh_get_kernel")
        return k.value

    def reserve_stream(self, stream: int, m: int, n: int, k: int) -> None:
        """Give `stream` (a raw hipStream_t) a stream-K workspace set of its own, large enough for any launch of an
        m x n x k problem: what a launch that is to be CAPTURED on that stream needs (include/mmult_hip.h, hipGraphs)."""
        _check(lib().mmh_reserve_stream(self._h, stream, m, n, k), "mmh_reserve_stream")

    def set_streamk(self, on) -> None:
        """False / 0 never, True / 1 when a round would be > 7 % empty (default), 2 whenever ragged."""
        _check(lib().mmh_set_option(self._h, OPT_STREAMK, int(on)), "mmh_set_option")

    def set_igemm_mode(self, mode: int) -> None:
        """By value and name in csrc/igemm_plan.hpp's mode table (kI8Modes): 0 "auto" B read in place (default; dense copies
        of unaligned operands first): the ping-pong 256x256 kernel K3p where its rounds of tiles are cheaper, 128x128 tiles of
        K3t otherwise; 2 "simple" the correctness-first kernel; 5 / 6 "k3t_128" / "k3t_256" the lockstep in-place kernel; 7
        "k3p_mfma32", 8 "k3p_persistent", 9 "k3p_per_tile" the ping-pong kernel on the 32-deep MFMA / as a persistent launch / one
        workgroup per tile.  (1 "k3", 3 / 4 "k3d_128" / "k3d_256" and 10..13, timing-only ablations with wrong results, exist
        only in the tools build libmmult_hip_ab.so; the product library rejects them.)  igemm_plan says what a call will run."""
        _check(lib().mmh_set_option(self._h, OPT_IGEMM_MODE, int(mode)), "mmh_set_option")

    def streamk_timeouts(self) -> int:
        """Synchronises; the handle's sticky error count: stream-K / split-K hand-off waits that timed
        out since it was last cleared (must be 0; while it is not, every call on the handle raises)."""
        v = C.c_int(0)
        _check(lib().mmh_get_option(self._h, OPT_STREAMK_TIMEOUTS, C.byref(v)), "mmh_get_option")
        return v.value

    def clear_error(self) -> None:
        """Synchronises and clears the sticky error."""
        _check(lib().mmh_set_option(self._h, OPT_STREAMK_TIMEOUTS, 0), "mmh_set_option")

    def set_option(self, option: int, value: int) -> None:
        _check(lib().mmh_set_option(self._h, int(option), int(value)), "mmh_set_option")

    def get_option(self, option: int) -> int:
        v = C.c_int(0)
        _check(lib().mmh_get_option(self._h, int(option), C.byref(v)), "mmh_get_option")
        return v.value

    def set_splitk(self, parts: int) -> None:
        """OPT-IN split-K for MMH_KERNEL_AUTO: 0 off (default), 1 as many parts as fill the chip,
        2..16 that many.  Deterministic, inside the harness tolerance, NOT the chain's bits."""
        self.set_option(OPT_SPLITK, parts)

    def set_host_panels(self, panels: int) -> None:
        """Row panels of the host flavour's copy/compute pipeline: -1 automatic, 0/1 plain, 2..16."""
        self.set_option(OPT_HOST_PANELS, panels)

    def device_info(self) -> dict:
        name = C.create_string_buffer(256)
        cu, mhz = C.c_int(0), C.c_int(0)
        _check(lib().mmh_device_info(self.device, name, C.byref(cu), C.byref(mhz)), "mmh_device_info")
        return {"name": name.value.decode(), "cu_count": cu.value, "clock_mhz": mhz.value}

    # -- the hot path, raw-pointer form (device flavour of MY_MMult) ---------
    def sgemm(self, m, n, k, dA: int, lda, dB: int, ldb, dC: int, ldc, accumulate=False,
              stream: int = 0) -> None:
        _check(lib().mmh_sgemm(self._h, m, n, k, dA, lda, dB, ldb, dC, ldc, int(bool(accumulate)),
                               stream), "mmh_sgemm")

    def sgemm_op(self, transa, transb, m, n, k, dA: int, lda, dB: int, ldb, dC: int, ldc, accumulate=False,
                 stream: int = 0) -> None:
        """C = op(A) op(B) (+ C), row-major: transa = OP_T reads A stored k x m (lda >= m), transb = OP_T B stored n x k
        (ldb >= k).  (OP_N, OP_N) is sgemm."""
        _check(lib().mmh_sgemm_op(self._h, int(transa), int(transb), m, n, k, dA, lda, dB, ldb, dC, ldc, int(bool(accumulate)),
                                  stream), "mmh_sgemm_op")

    def sgemm_ex(self, transa, transb, m, n, k, alpha, dA: int, lda, dB: int, ldb, beta, dC: int, ldc, dBias: int = 0,
                 bias_mode: int = BIAS_NONE, activation: int = ACT_NONE, stream: int = 0) -> None:
        """C = act(alpha op(A) op(B) + beta C + bias) in one launch, row-major device pointers as sgemm_op (include/mmult_hip.h,
        mmh_sgemm_ex: every rounding is defined there).  beta == 0: C is not read."""
        _check(lib().mmh_sgemm_ex(self._h, int(transa), int(transb), m, n, k, float(alpha), dA, lda, dB, ldb, float(beta), dC, ldc,
                                  dBias or None, int(bias_mode), int(activation), stream), "mmh_sgemm_ex")

    def sgemm_batched(self, transa, transb, m, n, k, dA: int, lda, stride_a, dB: int, ldb, stride_b, dC: int, ldc, stride_c,
                      batch, accumulate=False, stream: int = 0) -> None:
        """C_i = op(A_i) op(B_i) (+ C_i) for i < batch, row-major as sgemm_op; matrix i at dA + i stride_a (elements), and
        so on.  A stride of 0 broadcasts an operand; C matrices must not overlap (include/mmult_hip.h)."""
        _check(lib().mmh_sgemm_batched(self._h, int(transa), int(transb), m, n, k, dA, lda, stride_a, dB, ldb, stride_b, dC, ldc,
                                       stride_c, batch, int(bool(accumulate)), stream), "mmh_sgemm_batched")

    def sgemm_batched_ex(self, transa, transb, m, n, k, alpha, dA: int, lda, stride_a, dB: int, ldb, stride_b, beta, dC: int, ldc,
                         stride_c, batch, dBias: int = 0, stride_bias: int = 0, bias_mode: int = BIAS_NONE,
                         activation: int = ACT_NONE, stream: int = 0) -> None:
        """C_i = act(alpha op(A_i) op(B_i) + beta C_i + bias_i) for i < batch in one call (include/mmult_hip.h,
        mmh_sgemm_batched_ex): per matrix what sgemm_ex computes on it alone.  stride_bias: elements between two matrices'
        biases, 0 = one bias for the whole batch."""
        _check(lib().mmh_sgemm_batched_ex(self._h, int(transa), int(transb), m, n, k, float(alpha), dA, lda, stride_a, dB, ldb,
                                          stride_b, float(beta), dC, ldc, stride_c, dBias or None, stride_bias, int(bias_mode),
                                          int(activation), batch, stream), "mmh_sgemm_batched_ex")

    def MY_MMult_device(self, m, n, k, d_A: int, lda, d_B: int, ldb, d_C: int, ldc, stream: int = 0):
        """cuda/test_MMult.cpp:102 -- MY_MMult(handle, m, n, k, d_A, k, d_B, n, d_C, n):
        C = A*B on device pointers, asynchronous."""
        self.sgemm(m, n, k, d_A, lda, d_B, ldb, d_C, ldc, False, stream)

    # -- host flavour ----------------------------------------------------------
    def MY_MMult(self, m, n, k, a: np.ndarray, lda, b: np.ndarray, ldb, c: np.ndarray, ldc) -> None:
        """armv7/MMult0.c:9-24 semantics on host buffers: C = A*B + C (the caller
        pre-zeroes C, armv7/test_MMult.c:57,71).  a, b, c are flat or 2-D fp32
        numpy buffers addressed row-major with the given leading dimensions."""
        for x in (a, b, c):
            if x.dtype != np.float32 or not x.flags["C_CONTIGUOUS"]:
                raise MMultError(ERR_INVALID_ARG, "MY_MMult", "need C-contiguous float32 buffers")
        if k > 0 and m > 0 and (a.size < (m - 1) * lda + k or b.size < (k - 1) * ldb + n):
            raise MMultError(ERR_INVALID_ARG, "MY_MMult", "input buffer smaller than (rows-1)*ld+cols")
        if m > 0 and n > 0 and c.size < (m - 1) * ldc + n:
            raise MMultError(ERR_INVALID_ARG, "MY_MMult", "C buffer smaller than (m-1)*ldc+n")
        _check(lib().mmh_sgemm_host(self._h, m, n, k, _np_ptr(a), lda, _np_ptr(b), ldb, _np_ptr(c),
                                    ldc, 1), "mmh_sgemm_host")

    def MY_MMult_ms(self, m, n, k, a: np.ndarray, b: np.ndarray, c: np.ndarray) -> float:
        """vulkan/test_MMult.cpp:10,55 semantics: dense row-major host buffers (lda = k, ldb = n,
        ldc = n), C = A*B, returns the device time of the GEMM in milliseconds."""
        for x in (a, b, c):
            if x.dtype != np.float32 or not x.flags["C_CONTIGUOUS"]:
                raise MMultError(ERR_INVALID_ARG, "MY_MMult_ms", "need C-contiguous float32 buffers")
        if a.size < m * k or b.size < k * n or c.size < m * n:
            raise MMultError(ERR_INVALID_ARG, "MY_MMult_ms", "buffer smaller than rows*cols")
        ms = C.c_float(0.0)
        _check(lib().mmh_sgemm_host_timed(self._h, m, n, k, _np_ptr(a), max(k, 1), _np_ptr(b), max(n, 1),
                                          _np_ptr(c), max(n, 1), 0, C.byref(ms)), "mmh_sgemm_host_timed")
        return float(ms.value)

    def sgemm_host(self, a: np.ndarray, b: np.ndarray, c: Optional[np.ndarray] = None,
                   accumulate: bool = False) -> np.ndarray:
        m, k = a.shape
        k2, n = b.shape
        if k != k2:
            raise MMultError(ERR_INVALID_ARG, "sgemm_host", "inner dimensions differ")
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        if c is None:
            if accumulate:
                raise MMultError(ERR_INVALID_ARG, "sgemm_host", "accumulate needs c=")
            c = np.zeros((m, n), dtype=np.float32)
        elif (not isinstance(c, np.ndarray) or c.dtype != np.float32 or not c.flags["C_CONTIGUOUS"]
              or not c.flags["WRITEABLE"] or c.shape != (m, n)):
            raise MMultError(ERR_INVALID_ARG, "sgemm_host", f"c must be a writable C-contiguous float32 ({m},{n}) array")
        _check(lib().mmh_sgemm_host(self._h, m, n, k, _np_ptr(a), max(k, 1), _np_ptr(b), max(n, 1),
                                    _np_ptr(c), max(n, 1), int(accumulate)), "mmh_sgemm_host")
        return c

    # -- torch device-tensor glue (device memory + streams only) -------------
    def _tensor_args(self, t, rows, cols, what, dtype):
        """(data_ptr, leading dimension) of a (rows, cols) row-major window, after checking what the
        kernels take on trust: dtype, device (the handle's), unit column stride, and a row stride
        that does not fold rows onto each other (an expanded / overlapping view has stride(0) < cols)."""
        if not t.is_cuda:
            raise MMultError(ERR_INVALID_ARG, what, "tensor is not on a GPU (no CPU fallback)")
        if t.dtype != dtype:
            raise MMultError(ERR_INVALID_ARG, what, f"need dtype {dtype}, got {t.dtype}")
        if t.device.index != self.device:
            raise MMultError(ERR_INVALID_ARG, what,
                             f"tensor lives on cuda:{t.device.index}, the handle on cuda:{self.device}")
        if t.dim() != 2 or t.shape[0] != rows or t.shape[1] != cols or (cols > 1 and t.stride(1) != 1):
            raise MMultError(ERR_INVALID_ARG, what, f"need a ({rows},{cols}) row-major 2-D tensor")
        if rows > 1 and t.stride(0) < max(cols, 1):
            raise MMultError(ERR_INVALID_ARG, what,
                             f"row stride {t.stride(0)} < {cols} columns: rows overlap (expanded view?)")
        ld = t.stride(0) if rows > 1 else max(cols, 1)
        return t.data_ptr(), max(ld, 1)

    def _operand_args(self, t, rows, cols, what):
        """(data_ptr, leading dimension, OP_N / OP_T) of a matmul operand: a row-major window as _tensor_args takes it,
        or else a TRANSPOSED view -- stride(0) == 1, stride(1) >= rows (w.t(), a .t() of a row-strided window) --, whose
        .t() is such a window.  A tensor both readings take (one row or one column) is read row-major."""
        import torch
        try:
            return self._tensor_args(t, rows, cols, what, torch.float32) + (OP_N,)
        except MMultError:
            if not (t.dim() == 2 and tuple(t.shape) == (rows, cols) and cols > 1 and (rows <= 1 or t.stride(0) == 1)
                    and t.stride(1) >= max(rows, 1)):
                raise
        return self._tensor_args(t.t(), cols, rows, what, torch.float32) + (OP_T,)

    def _shapes_and_out(self, what, a, b, out, out_dtype, accumulate=False):
        """(m, n, k) of a 2-D a @ b after the inner-dimension check, and `out`: the caller's, or a new (m, n) tensor beside a."""
        import torch
        m, k = a.shape
        k2, n = b.shape
        if k != k2:
            raise MMultError(ERR_INVALID_ARG, what, "inner dimensions differ")
        if out is None:
            if accumulate:
                raise MMultError(ERR_INVALID_ARG, what, "accumulate needs out=")
            out = torch.empty((m, n), dtype=out_dtype, device=a.device)
        return m, n, k, out

    def _gemm_2d(self, what, label, a, b, out, in_dtype, out_dtype, accumulate=False):
        """The front end of the 2-D calls on row-major windows: _shapes_and_out, then A, B and C through _tensor_args -- errors
        name them label(A), label(B), label(C) -- and torch's current stream.  Returns the C functions' (m, n, k, A, lda, B, ldb,
        C, ldc), the stream, and out."""
        import torch
        m, n, k, out = self._shapes_and_out(what, a, b, out, out_dtype, accumulate)
        pa, lda = self._tensor_args(a, m, k, label + "(A)", in_dtype)
        pb, ldb = self._tensor_args(b, k, n, label + "(B)", in_dtype)
        pc, ldc = self._tensor_args(out, m, n, label + "(C)", out_dtype)
        return (m, n, k, pa, lda, pb, ldb, pc, ldc), torch.cuda.current_stream(a.device).cuda_stream, out

    def matmul(self, a, b, out=None, accumulate: bool = False):
        """C = A @ B (+ C) for fp32 CUDA tensors, on torch's current stream.  A and B may be transposed views (x @ w.t(),
        a.t() @ b): they are read in place through mmh_sgemm_op; `out` is row-major."""
        import torch
        if a.dtype != torch.float32 or b.dtype != torch.float32:
            raise MMultError(ERR_INVALID_ARG, "matmul", "fp32 only")
        m, n, k, out = self._shapes_and_out("matmul", a, b, out, torch.float32, accumulate)
        pa, lda, ta = self._operand_args(a, m, k, "matmul(A)")
        pb, ldb, tb = self._operand_args(b, k, n, "matmul(B)")
        pc, ldc = self._tensor_args(out, m, n, "matmul(C)", torch.float32)
        stream = torch.cuda.current_stream(a.device).cuda_stream
        if ta == OP_N and tb == OP_N:
            self.sgemm(m, n, k, pa, lda, pb, ldb, pc, ldc, accumulate, stream)
        else:
            self.sgemm_op(ta, tb, m, n, k, pa, lda, pb, ldb, pc, ldc, accumulate, stream)
        return out

    def _ex_args(self, what, a, b, out):
        """_ex's operands after its checks: (m, n, k, pa, lda, ta, pb, ldb, tb, pc, ldc).  addmm asks before it copies `input` into
        `out`: nothing is written to the `out` of a call that will be refused."""
        import torch
        if a.dtype != torch.float32 or b.dtype != torch.float32:
            raise MMultError(ERR_INVALID_ARG, what, "fp32 only")
        if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[0]:
            raise MMultError(ERR_INVALID_ARG, what, "need 2-D operands whose inner dimensions agree")
        (m, k), n = a.shape, b.shape[1]
        return (m, n, k) + self._operand_args(a, m, k, what + "(A)") + self._operand_args(b, k, n, what + "(B)") + \
            self._tensor_args(out, m, n, what + "(C)", torch.float32)

    def _ex(self, what, a, b, out, alpha, beta, bias, bias_mode, activation):
        """out = act(alpha a @ b + beta out + bias) through mmh_sgemm_ex on torch's current stream; a / b as matmul takes them."""
        import torch
        m, n, k, pa, lda, ta, pb, ldb, tb, pc, ldc = self._ex_args(what, a, b, out)
        pbias = 0
        if bias is not None:
            if not bias.is_cuda or bias.device.index != self.device or bias.dtype != torch.float32 or bias.dim() != 1 or \
                    bias.shape[0] != (n if bias_mode == BIAS_COL else m) or (bias.shape[0] > 1 and bias.stride(0) != 1):
                raise MMultError(ERR_INVALID_ARG, what, "the bias is a dense 1-D fp32 tensor on the handle's device, one float per "
                                 "output column")
            pbias = bias.data_ptr()
        # (a bias of no floats -- no output column -- has nothing to add, and no pointer to pass: torch gives an empty tensor NULL)
        stream = torch.cuda.current_stream(a.device).cuda_stream
        self.sgemm_ex(ta, tb, m, n, k, alpha, pa, lda, pb, ldb, beta, pc, ldc, pbias, bias_mode if pbias else BIAS_NONE, activation,
                      stream)
        return out

    def addmm(self, input, a, b, *, beta=1.0, alpha=1.0, out=None):
        """torch.addmm: out = beta input + alpha a @ b in ONE launch (mmh_sgemm_ex: fl(fl(alpha s) + fl(beta input)), s the fp32
        fma chain).  `input` (m, n): in place when `out is input`, otherwise copied into `out` first; `input` (n,) with
        beta == 1: the kernel's column bias (no copy); any other 1-D `input` is broadcast into `out` first.  a, b may be
        transposed views, read in place."""
        import torch
        if a.dim() != 2 or b.dim() != 2:
            raise MMultError(ERR_INVALID_ARG, "addmm", "need 2-D operands")
        m, n = a.shape[0], b.shape[1]
        if input.dim() == 1 and input.shape[0] == n and float(beta) == 1.0 and out is not input:
            if out is None:
                out = torch.empty((m, n), dtype=torch.float32, device=a.device)
            return self._ex("addmm", a, b, out, alpha, 0.0, input, BIAS_COL, ACT_NONE)
        if input.dim() == 1 and input.shape[0] != n or input.dim() == 2 and tuple(input.shape) != (m, n) or input.dim() not in (1, 2):
            raise MMultError(ERR_INVALID_ARG, "addmm", f"input must be ({m},{n}) or ({n},)")
        if out is None:
            out = torch.empty((m, n), dtype=torch.float32, device=a.device)
        if out is not input:
            if float(beta) != 0.0:
                self._ex_args("addmm", a, b, out)   # (nothing is copied into the `out` of a call that will be refused)
                out.copy_(input)   # (1-D: broadcast over the rows)
        return self._ex("addmm", a, b, out, alpha, beta, None, BIAS_NONE, ACT_NONE)

    def linear(self, x, w, bias=None, activation=None, out=None):
        """torch.nn.functional.linear (+ ReLU) in ONE launch: y = act(x @ w.t() + bias), `w` stored out x in and read in place
        (NT), `bias` (out,), activation None or "relu"."""
        import torch
        if activation not in (None, "relu"):
            raise MMultError(ERR_INVALID_ARG, "linear", "activation is None or 'relu'")
        if x.dim() != 2 or w.dim() != 2:
            raise MMultError(ERR_INVALID_ARG, "linear", "need a 2-D x (batch, in) and a 2-D w (out, in)")
        if out is None:
            out = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32, device=x.device)
        return self._ex("linear", x, w.t(), out, 1.0, 0.0, bias, BIAS_COL, ACT_RELU if activation == "relu" else ACT_NONE)

    # -- the linear layer's backward (mmh_relu_grad_colsum + the GEMMs that are already there) --------------------------
    def _relu_grad_args(self, what, g, y, dz, want_dz, bias_grad, want_colsum, accumulate):
        """The C call's arguments for relu_grad_colsum / time_relu_grad_colsum, outputs allocated: (rows, cols, pg, ldg, py, ldy,
        pz, ldz, pcolsum, accumulate), dz, colsum."""
        import torch
        if g.dim() != 2:
            raise MMultError(ERR_INVALID_ARG, what, "need a 2-D gradient (rows, cols)")
        rows, cols = g.shape
        pg, ldg = self._tensor_args(g, rows, cols, what + "(g)", torch.float32)
        py, ldy = (0, max(cols, 1)) if y is None else self._tensor_args(y, rows, cols, what + "(y)", torch.float32)
        if dz is None and want_dz:
            dz = torch.empty((rows, cols), dtype=torch.float32, device=g.device)
        pz, ldz = (0, max(cols, 1)) if dz is None else self._tensor_args(dz, rows, cols, what + "(dz)", torch.float32)
        colsum = bias_grad
        if colsum is None and want_colsum:
            if accumulate:
                raise MMultError(ERR_INVALID_ARG, what, "accumulate needs bias_grad=")
            colsum = torch.empty((cols,), dtype=torch.float32, device=g.device)
        if colsum is not None and (not colsum.is_cuda or colsum.device.index != self.device or colsum.dtype != torch.float32 or
                                   colsum.dim() != 1 or colsum.shape[0] != cols or (cols > 1 and colsum.stride(0) != 1)):
            raise MMultError(ERR_INVALID_ARG, what, f"bias_grad is a dense 1-D fp32 tensor of {cols} floats on the handle's device")
        if dz is None and colsum is None:
            raise MMultError(ERR_INVALID_ARG, what, "nothing to compute: neither dz nor the column sum is wanted")
        args = (rows, cols, pg, ldg, py or None, ldy, pz or None, ldz, colsum.data_ptr() if colsum is not None else None,
                int(bool(accumulate)))
        return args, dz, colsum

    def relu_grad_colsum(self, g, y=None, *, dz=None, want_dz=True, bias_grad=None, want_colsum=True, accumulate=False):
        """The memory-bound pass of a linear layer's backward, ONE launch (mmh_relu_grad_colsum; every rounding is defined in
        include/mmult_hip.h) on torch's current stream: dz = g where y > 0 (dz = g without y) and colsum = the column sums of
        dz in blocks of COLSUM_BLOCK_ROWS rows.  g, y (the forward OUTPUT), dz: (rows, cols) row-major windows; dz=g works in
        place; want_dz=False / want_colsum=False skip an output; bias_grad= receives the sums (accumulate=True: adds them).
        Returns (dz or None, colsum or None)."""
        import torch
        args, dz, colsum = self._relu_grad_args("relu_grad_colsum", g, y, dz, want_dz, bias_grad, want_colsum, accumulate)
        rows, cols = args[0], args[1]
        if cols == 0:
            return dz, colsum
        if rows == 0:   # (an empty tensor has no pointer to pass: the empty sum is +0)
            if colsum is not None and not accumulate:
                colsum.zero_()
            return dz, colsum
        stream = torch.cuda.current_stream(g.device).cuda_stream
        _check(lib().mmh_relu_grad_colsum(self._h, *args, stream), "mmh_relu_grad_colsum")
        return dz, colsum

    def time_relu_grad_colsum(self, g, y=None, *, dz=None, want_dz=True, bias_grad=None, want_colsum=True, accumulate=False,
                              warmup=1, reps=20) -> float:
        """time_sgemm for relu_grad_colsum (same arguments): mean ms per call, one event pair on torch's current stream."""
        import torch
        args, _, _ = self._relu_grad_args("time_relu_grad_colsum", g, y, dz, want_dz, bias_grad, want_colsum, accumulate)
        if args[0] == 0 or args[1] == 0:   # (an empty tensor has no pointer to pass; relu_grad_colsum launches nothing either)
            raise MMultError(ERR_INVALID_ARG, "time_relu_grad_colsum", "nothing to time: the gradient is empty")
        return self._time("mmh_time_relu_grad_colsum", *args, warmup, reps, torch.cuda.current_stream(g.device).cuda_stream)

    def linear_backward(self, grad_out, x, w, y=None, *, need=(True, True, True), grad_w=None, grad_b=None):
        """The backward of linear(x, w, b) (+ ReLU when `y`, the forward output, is given): (dx, dw, db) for the incoming
        gradient grad_out (rows, out), x (rows, in), w (out, in).  One relu_grad_colsum call -- it gates when y is given, sums
        the columns when need[2], and writes dz only when a GEMM needs it and y is given (without y, dz IS grad_out) -- then
        dx = dz @ w (sgemm) and dw = dz.t() @ x (sgemm_op, TN).  grad_w= / grad_b= accumulate in place: fl(grad_w + s) with s
        the whole TN chain (sgemm_ex, beta = 1: torch's `+=`, not the chain started at grad_w), fl(grad_b + colsum).  Entries
        of `need` that are False give None and cost no launch.  Every launch is on torch's current stream."""
        import torch
        need_x, need_w, need_b = (bool(v) for v in need)
        if grad_out.dim() != 2 or x.dim() != 2 or w.dim() != 2 or grad_out.shape[0] != x.shape[0] or \
                tuple(w.shape) != (grad_out.shape[1], x.shape[1]):
            raise MMultError(ERR_INVALID_ARG, "linear_backward", "need grad_out (rows, out), x (rows, in) and w (out, in)")
        rows, n_out, n_in = grad_out.shape[0], grad_out.shape[1], x.shape[1]
        pg, ldg = self._tensor_args(grad_out, rows, n_out, "linear_backward(grad_out)", torch.float32)
        px, ldx = self._tensor_args(x, rows, n_in, "linear_backward(x)", torch.float32)
        pw, ldw = self._tensor_args(w, n_out, n_in, "linear_backward(w)", torch.float32)
        if y is not None:
            self._tensor_args(y, rows, n_out, "linear_backward(y)", torch.float32)
        if grad_w is not None:
            pgw, ldgw = self._tensor_args(grad_w, n_out, n_in, "linear_backward(grad_w)", torch.float32)
        if need_w:
            # a selected kernel without op / ex forms refuses before anything is launched (the plan is host arithmetic)
            kern = self.get_kernel()
            if lib().mmh_kernel_has_op_forms(kern) != 1:
                raise MMultError(ERR_UNSUPPORTED, "linear_backward",
                                 f"the selected kernel {kernel_name(kern)} has no transposed-operand form for dw = dz.t() @ x")
        dev = grad_out.device
        gemm = need_x or need_w
        dz, db = grad_out, None
        if need_b or (gemm and y is not None):
            dz_, db = self.relu_grad_colsum(grad_out, y, want_dz=gemm and y is not None, bias_grad=grad_b if need_b else None,
                                            want_colsum=need_b, accumulate=need_b and grad_b is not None)
            if dz_ is not None:
                dz = dz_
        stream = torch.cuda.current_stream(dev).cuda_stream
        dx = dw = None
        pz, ldz = (dz.data_ptr(), max(dz.stride(0) if rows > 1 else n_out, 1)) if dz is not grad_out else (pg, ldg)
        if need_x:
            dx = torch.empty((rows, n_in), dtype=torch.float32, device=dev)
            self.sgemm(rows, n_in, n_out, pz, ldz, pw, ldw, dx.data_ptr(), max(n_in, 1), False, stream)
        if need_w:
            if grad_w is None:
                dw = torch.empty((n_out, n_in), dtype=torch.float32, device=dev)
                self.sgemm_op(OP_T, OP_N, n_out, n_in, rows, pz, ldz, px, ldx, dw.data_ptr(), max(n_in, 1), False, stream)
            else:
                dw = grad_w
                self.sgemm_ex(OP_T, OP_N, n_out, n_in, rows, 1.0, pz, ldz, px, ldx, 1.0, pgw, ldgw, stream=stream)
        return dx, dw, db

    def _batched_args(self, t, batch, rows, cols, what, operand):
        """(data_ptr, leading dimension, op, batch stride) of a 3-D (batch, rows, cols) tensor: each matrix a row-major
        window or (operands only) a transposed view, as matmul takes them; any batch stride >= 0 (expand() gives 0)."""
        import torch
        if t.dim() != 3 or tuple(t.shape) != (batch, rows, cols):
            raise MMultError(ERR_INVALID_ARG, what, f"need a ({batch},{rows},{cols}) 3-D tensor")
        if batch == 0:
            return 0, max(cols, 1), OP_N, 0
        if operand:
            p, ld, op = self._operand_args(t[0], rows, cols, what)
        else:
            p, ld = self._tensor_args(t[0], rows, cols, what, torch.float32)
            op = OP_N
        return p, ld, op, (t.stride(0) if batch > 1 else 0)

    def bmm(self, a, b, out=None, accumulate: bool = False):
        """C[i] = A[i] @ B[i] (+ C[i]) for 3-D fp32 CUDA tensors [batch, m, k] @ [batch, k, n], on torch's current stream,
        through mmh_sgemm_batched.  Each operand's matrices may be row-major or transposed views (x.transpose(1, 2)), with
        any batch stride >= 0 (expand() broadcasts); `out` is row-major per matrix, its matrices must not overlap."""
        import torch
        if a.dtype != torch.float32 or b.dtype != torch.float32:
            raise MMultError(ERR_INVALID_ARG, "bmm", "fp32 only")
        if a.dim() != 3 or b.dim() != 3:
            raise MMultError(ERR_INVALID_ARG, "bmm", "need 3-D tensors")
        batch, m, k = a.shape
        b2, k2, n = b.shape
        if k != k2 or batch != b2:
            raise MMultError(ERR_INVALID_ARG, "bmm", "batch or inner dimensions differ")
        if out is None:
            if accumulate:
                raise MMultError(ERR_INVALID_ARG, "bmm", "accumulate needs out=")
            out = torch.empty((batch, m, n), dtype=torch.float32, device=a.device)
        pa, lda, ta, sa = self._batched_args(a, batch, m, k, "bmm(A)", True)
        pb, ldb, tb, sb = self._batched_args(b, batch, k, n, "bmm(B)", True)
        pc, ldc, _, sc = self._batched_args(out, batch, m, n, "bmm(C)", False)
        if batch == 0:
            return out
        stream = torch.cuda.current_stream(a.device).cuda_stream
        self.sgemm_batched(ta, tb, m, n, k, pa, lda, sa, pb, ldb, sb, pc, ldc, sc, batch, accumulate, stream)
        return out

    def _batched_ex_args(self, what, a, b, out):
        """_batched_ex's operands after its checks: (batch, m, n, k) and _batched_args of a, b and out.  baddbmm asks before it
        copies `input` into `out`."""
        import torch
        if a.dtype != torch.float32 or b.dtype != torch.float32:
            raise MMultError(ERR_INVALID_ARG, what, "fp32 only")
        if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[2] != b.shape[1]:
            raise MMultError(ERR_INVALID_ARG, what, "need 3-D operands whose batch and inner dimensions agree")
        (batch, m, k), n = a.shape, b.shape[2]
        return (batch, m, n, k), self._batched_args(a, batch, m, k, what + "(A)", True), \
            self._batched_args(b, batch, k, n, what + "(B)", True), self._batched_args(out, batch, m, n, what + "(C)", False)

    def _batched_ex(self, what, a, b, out, alpha, beta, bias, stride_bias, activation):
        """out[i] = act(alpha a[i] @ b[i] + beta out[i] + bias_i) through mmh_sgemm_batched_ex on torch's current stream; a / b /
        out as bmm takes them; bias: None, or a column bias -- a tensor whose n floats per matrix are dense, matrix i's
        stride_bias elements behind matrix i - 1's."""
        import torch
        (batch, m, n, k), (pa, lda, ta, sa), (pb, ldb, tb, sb), (pc, ldc, _, sc) = self._batched_ex_args(what, a, b, out)
        pbias = 0
        if bias is not None:
            if not bias.is_cuda or bias.device.index != self.device or bias.dtype != torch.float32 or stride_bias < 0 or \
                    (n > 1 and bias.stride(-1) != 1):
                raise MMultError(ERR_INVALID_ARG, what, "the bias is an fp32 tensor on the handle's device, one dense run of floats per "
                                 "matrix, one float per output column")
            pbias = bias.data_ptr()
        if batch == 0:
            return out
        stream = torch.cuda.current_stream(a.device).cuda_stream
        # (a bias of no floats -- no output column -- has nothing to add, and no pointer to pass: torch gives an empty tensor NULL)
        self.sgemm_batched_ex(ta, tb, m, n, k, alpha, pa, lda, sa, pb, ldb, sb, beta, pc, ldc, sc, batch, pbias, stride_bias,
                              BIAS_COL if pbias else BIAS_NONE, activation, stream)
        return out

    def baddbmm(self, input, a, b, *, beta=1.0, alpha=1.0, out=None):
        """torch.baddbmm: out[i] = beta input[i] + alpha a[i] @ b[i] in ONE call (mmh_sgemm_batched_ex), addmm's rules per matrix.
        `input` (batch, m, n): in place when `out is input`, otherwise copied into `out` first (not when beta == 0; out.copy_
        broadcasts any shape torch broadcasts); `input` (n,) or (batch, 1, n) with beta == 1: the kernel's column bias, shared
        or per matrix (no copy).  a, b as bmm takes them: transposed views, expand()ed batches."""
        import torch
        if a.dim() != 3 or b.dim() != 3:
            raise MMultError(ERR_INVALID_ARG, "baddbmm", "need 3-D operands")
        batch, m, n = a.shape[0], a.shape[1], b.shape[2]
        if float(beta) == 1.0 and out is not input and n >= 1 and (
                (input.dim() == 1 and input.shape[0] == n) or
                (input.dim() == 3 and tuple(input.shape) == (batch, 1, n))):
            if out is None:
                out = torch.empty((batch, m, n), dtype=torch.float32, device=a.device)
            stride_bias = input.stride(0) if input.dim() == 3 and batch > 1 else 0
            return self._batched_ex("baddbmm", a, b, out, alpha, 0.0, input, stride_bias, ACT_NONE)
        if out is None:
            out = torch.empty((batch, m, n), dtype=torch.float32, device=a.device)
        if out is not input:
            try:
                fits = tuple(torch.broadcast_shapes(tuple(input.shape), (batch, m, n))) == (batch, m, n)
            except RuntimeError:
                fits = False
            if not fits:
                raise MMultError(ERR_INVALID_ARG, "baddbmm", f"input must broadcast to ({batch},{m},{n})")
            if float(beta) != 0.0:
                # (nothing is copied into the `out` of a call that will be refused: a CPU tensor, matrices that overlap, operands
                # that disagree or cannot be read)
                _, _, _, (_, ldc, _, sc) = self._batched_ex_args("baddbmm", a, b, out)
                if batch > 1 and sc < (m - 1) * ldc + n:
                    raise MMultError(ERR_INVALID_ARG, "baddbmm(C)", "the matrices of out overlap")
                if input.device != out.device:
                    raise MMultError(ERR_INVALID_ARG, "baddbmm", "input and out live on different devices")
                out.copy_(input)
        return self._batched_ex("baddbmm", a, b, out, alpha, beta, None, 0, ACT_NONE)

    def batched_linear(self, x, w, bias=None, activation=None, out=None):
        """A batch of equally shaped linear layers (+ ReLU) in ONE call: y[i] = act(x[i] @ w[i].t() + bias[i]).  x (batch, rows,
        in); w (batch, out, in), or (out, in) shared by the whole batch -- read in place (NT); bias (batch, out) or (out,);
        activation None or "relu"."""
        import torch
        if activation not in (None, "relu"):
            raise MMultError(ERR_INVALID_ARG, "batched_linear", "activation is None or 'relu'")
        if x.dim() != 3 or w.dim() not in (2, 3):
            raise MMultError(ERR_INVALID_ARG, "batched_linear", "need a 3-D x (batch, rows, in) and a w (batch, out, in) or (out, in)")
        batch = x.shape[0]
        if w.dim() == 2:
            w = w.unsqueeze(0).expand(batch, -1, -1)
        if w.shape[0] != batch:
            raise MMultError(ERR_INVALID_ARG, "batched_linear", "x and w differ in their batch")
        n = w.shape[1]
        stride_bias = 0
        if bias is not None:
            if bias.dim() == 2 and tuple(bias.shape) == (batch, n):
                stride_bias = bias.stride(0) if batch > 1 else 0
            elif not (bias.dim() == 1 and bias.shape[0] == n):
                raise MMultError(ERR_INVALID_ARG, "batched_linear", f"bias must be ({batch},{n}) or ({n},)")
        if out is None:
            out = torch.empty((batch, x.shape[1], n), dtype=torch.float32, device=x.device)
        return self._batched_ex("batched_linear", x, w.transpose(1, 2), out, 1.0, 0.0, bias, stride_bias,
                                ACT_RELU if activation == "relu" else ACT_NONE)

    def igemm_s8(self, a, b, out=None, accumulate: bool = False):
        """int8 x int8 -> int32 for CUDA tensors (any int8; every sum must fit in int32)."""
        import torch
        if a.dtype != torch.int8 or b.dtype != torch.int8:
            raise MMultError(ERR_INVALID_ARG, "igemm_s8", "int8 inputs only")
        args, stream, out = self._gemm_2d("igemm_s8", "igemm_s8", a, b, out, torch.int8, torch.int32, accumulate)
        _check(lib().mmh_igemm_s8(self._h, *args, int(accumulate), stream), "mmh_igemm_s8")
        return out

    def quantize_sym_s8(self, x):
        """fp32 CUDA tensor -> (int8 tensor in [-127,127], scale as a 1-element CUDA tensor)."""
        import torch
        if x.dim() != 2:
            raise MMultError(ERR_INVALID_ARG, "quantize(X)", "need a 2-D tensor")
        rows, cols = x.shape
        px, ldx = self._tensor_args(x, rows, cols, "quantize(X)", torch.float32)
        q = torch.empty((rows, cols), dtype=torch.int8, device=x.device)
        scale = torch.empty(1, dtype=torch.float32, device=x.device)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _check(lib().mmh_quantize_sym_s8(self._h, rows, cols, px, ldx, q.data_ptr(), max(cols, 1),
                                         scale.data_ptr(), stream), "mmh_quantize_sym_s8")
        return q, scale

    def qgemm(self, a, b, out=None):
        """C_f32 = dequantise(quantise(A) @ quantise(B)): chgemm-style symmetric int8 GEMM."""
        import torch
        args, stream, out = self._gemm_2d("qgemm", "qgemm", a, b, out, torch.float32, torch.float32)
        _check(lib().mmh_qgemm_f32(self._h, *args, stream), "mmh_qgemm_f32")
        return out

    def matmul_rocblas(self, a, b, out=None):
        """Vendor comparator (cuda/MMult_cuBLAS_1.cpp:11-19)."""
        import torch
        args, stream, out = self._gemm_2d("matmul_rocblas", "rocblas", a, b, out, torch.float32, torch.float32)
        _check(lib().mmh_sgemm_rocblas(self._h, *args, stream), "mmh_sgemm_rocblas")
        return out

    def matmul_hipblaslt(self, a, b, out=None):
        """The second vendor comparator (cuda/MMult_cuBLAS_2.cpp:11-26): hipBLASLt, fp32 compute."""
        import torch
        args, stream, out = self._gemm_2d("matmul_hipblaslt", "hipblaslt", a, b, out, torch.float32, torch.float32)
        _check(lib().mmh_sgemm_hipblaslt(self._h, *args, stream), "mmh_sgemm_hipblaslt")
        return out

    # -- measurement -------------------------------------------------------------
    def _time(self, name, *args) -> float:
        """The mmh_time_* function `name` on this handle: its arguments up to the result, which is returned (ms per call)."""
        ms = C.c_float(0.0)
        _check(getattr(lib(), name)(self._h, *args, C.byref(ms)), name)
        return float(ms.value)

    def time_sgemm(self, m, n, k, dA, lda, dB, ldb, dC, ldc, warmup=1, reps=20, stream: int = 0) -> float:
        """Mean ms per call: one hipEvent pair around `reps` back-to-back launches on
        `stream` (the reference's convention, cuda/test_MMult.cpp:98-114)."""
        return self._time("mmh_time_sgemm", m, n, k, dA, lda, dB, ldb, dC, ldc, warmup, reps, stream)

    def time_sgemm_op(self, transa, transb, m, n, k, dA, lda, dB, ldb, dC, ldc, warmup=1, reps=20, stream: int = 0) -> float:
        """time_sgemm for mmh_sgemm_op (every op pair, (OP_N, OP_N) included)."""
        return self._time("mmh_time_sgemm_op", int(transa), int(transb), m, n, k, dA, lda, dB, ldb, dC, ldc, warmup, reps, stream)

    def time_sgemm_ex(self, transa, transb, m, n, k, alpha, dA, lda, dB, ldb, beta, dC, ldc, dBias=0, bias_mode=BIAS_NONE,
                      activation=ACT_NONE, warmup=1, reps=20, stream: int = 0) -> float:
        """time_sgemm for mmh_sgemm_ex."""
        return self._time("mmh_time_sgemm_ex", int(transa), int(transb), m, n, k, float(alpha), dA, lda, dB, ldb, float(beta), dC, ldc,
                          dBias or None, int(bias_mode), int(activation), warmup, reps, stream)

    def time_sgemm_batched_ex(self, transa, transb, m, n, k, alpha, dA, lda, stride_a, dB, ldb, stride_b, beta, dC, ldc, stride_c,
                              batch, dBias=0, stride_bias=0, bias_mode=BIAS_NONE, activation=ACT_NONE, warmup=1, reps=20,
                              stream: int = 0) -> float:
        """time_sgemm for mmh_sgemm_batched_ex: ms per batched call."""
        return self._time("mmh_time_sgemm_batched_ex", int(transa), int(transb), m, n, k, float(alpha), dA, lda, stride_a, dB, ldb,
                          stride_b, float(beta), dC, ldc, stride_c, dBias or None, stride_bias, int(bias_mode), int(activation), batch,
                          warmup, reps, stream)

    def time_sgemm_batched(self, transa, transb, m, n, k, dA, lda, stride_a, dB, ldb, stride_b, dC, ldc, stride_c, batch,
                           warmup=1, reps=20, stream: int = 0) -> float:
        """time_sgemm for mmh_sgemm_batched: ms per batched call."""
        return self._time("mmh_time_sgemm_batched", int(transa), int(transb), m, n, k, dA, lda, stride_a, dB, ldb, stride_b, dC, ldc,
                          stride_c, batch, warmup, reps, stream)

    def time_comparator(self, which: str, m, n, k, dA, lda, dB, ldb, dC, ldc, warmup=1, reps=20, stream: int = 0) -> float:
        """time_sgemm for a vendor comparator ("rocblas" / "hipblaslt"): calls issued from C, one event pair."""
        return self._time("mmh_time_comparator", _abi.constants("MMH_COMPARATOR_")[which.upper()], m, n, k, dA, lda, dB, ldb, dC, ldc, warmup, reps,
                          stream)

    def trace_sgemm(self, m, n, k, dA, lda, dB, ldb, dC, ldc, count=400, stream: int = 0):
        """Per-launch ms of `count` back-to-back launches (one hipEvent pair each): the clock ramp."""
        buf = (C.c_float * count)()
        _check(lib().mmh_trace_sgemm(self._h, m, n, k, dA, lda, dB, ldb, dC, ldc, count, stream, buf),
               "mmh_trace_sgemm")
        return list(buf)

    def probe_mfma_f32(self) -> float:
        v = C.c_float(0)
        _check(lib().mmh_probe_mfma_f32(self._h, C.byref(v)), "mmh_probe_mfma_f32")
        return v.value

    def probe_valu_f32(self, packed: bool = True, waves_per_simd: int = 2) -> float:
        """TFLOP/s of a v_pk_fma_f32-only (packed) or v_fma_f32-only loop: the vector-ALU rung's measured roof."""
        v = C.c_float(0)
        _check(lib().mmh_probe_valu_f32(self._h, int(bool(packed)), int(waves_per_simd), C.byref(v)), "mmh_probe_valu_f32")
        return v.value

    def probe_mfma_i8(self) -> float:
        v = C.c_float(0)
        _check(lib().mmh_probe_mfma_i8(self._h, C.byref(v)), "mmh_probe_mfma_i8")
        return v.value

    def probe_mfma_i8_sustained(self, random_operands: bool = True, min_ms: float = 50.0) -> float:
        """int8 MFMA-only rate of the LAST 2.3 ms launch after `min_ms` of back-to-back launches,
        with per-MFMA pseudo-random operands (what the power manager sustains on real data) or
        with constant ones."""
        v = C.c_float(0)
        _check(lib().mmh_probe_mfma_i8_sustained(self._h, int(bool(random_operands)), float(min_ms), C.byref(v)),
               "mmh_probe_mfma_i8_sustained")
        return v.value

    def probe_hbm_copy(self, nbytes: int = 1 << 30) -> float:
        v = C.c_float(0)
        _check(lib().mmh_probe_hbm_copy(self._h, nbytes, C.byref(v)), "mmh_probe_hbm_copy")
        return v.value

    def probe_hbm_read(self, nbytes: int = 1 << 30) -> float:
        v = C.c_float(0)
        _check(lib().mmh_probe_hbm_read(self._h, nbytes, C.byref(v)), "mmh_probe_hbm_read")
        return v.value

    def probe_lds_read(self, width: int = 16) -> float:
        """LDS fragment-read rate summed over the chip, GB/s (width 16 / 8 / 4 bytes per lane, -8 = the
        transposing ds_read_b64_tr_b8)."""
        v = C.c_float(0.0)
        _check(lib().mmh_probe_lds_read(self._h, int(width), C.byref(v)), "mmh_probe_lds_read")
        return float(v.value)


class ShardedMMult:
    """Single-process row-panel shard over `ngpus` devices with everything persistent (one RCCL
    communicator, per-device streams, product handles and buffers): mmh_shard_create/_sgemm/_destroy.
    Raises MMultError(ERR_NO_DEVICE) when fewer devices are visible -- never fewer ranks silently."""

    def __init__(self, ngpus: int, devices=None, kernel="auto"):
        self._h = C.c_void_p(None)
        dev = None
        if devices is not None:
            if len(devices) != ngpus:
                raise MMultError(ERR_INVALID_ARG, "ShardedMMult", "len(devices) != ngpus")
            dev = (C.c_int * ngpus)(*devices)
        _check(lib().mmh_shard_create(C.byref(self._h), ngpus, dev), "mmh_shard_create")
        _check(lib().mmh_shard_set_kernel(self._h, _kernel_id(kernel)), "mmh_shard_set_kernel")

    def close(self) -> None:
        if self._h:
            lib().mmh_shard_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self) -> dict:
        n, r = C.c_int(0), C.c_int(0)
        _check(lib().mmh_shard_info(self._h, C.byref(n), C.byref(r)), "mmh_shard_info")
        return {"ngpus": n.value, "rccl_ranks": r.value}

    def pin(self, x: np.ndarray) -> None:
        """Page-lock a host array that will be passed to sgemm() repeatedly (unpin before it is freed)."""
        _check(lib().mmh_shard_pin(self._h, _np_ptr(x), x.nbytes), "mmh_shard_pin")

    def unpin(self, x: np.ndarray) -> None:
        _check(lib().mmh_shard_unpin(self._h, _np_ptr(x)), "mmh_shard_unpin")

    def sgemm(self, a: np.ndarray, b: np.ndarray, c: Optional[np.ndarray] = None, gemm_reps: int = 1, b_chunks: int = 1):
        """C = A @ B on host arrays.  Returns (C, {"h2d","bcast","gemm","d2h"} ms; gemm is per rep); with b_chunks > 1
        (mmh_shard_sgemm_streamed: B broadcast in K-chunks under the GEMMs that consume them) also "overlapped",
        "chunks", "first_pass", "wall"."""
        m, k = a.shape
        k2, n = b.shape
        if k != k2:
            raise MMultError(ERR_INVALID_ARG, "ShardedMMult.sgemm", "inner dimensions differ")
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        if c is None:
            c = np.zeros((m, n), dtype=np.float32)
        elif c.dtype != np.float32 or not c.flags["C_CONTIGUOUS"] or c.shape != (m, n):
            raise MMultError(ERR_INVALID_ARG, "ShardedMMult.sgemm", "c must be C-contiguous float32 (m,n)")
        if b_chunks > 1:
            t = (C.c_float * 8)()
            _check(lib().mmh_shard_sgemm_streamed(self._h, m, n, k, _np_ptr(a), max(k, 1), _np_ptr(b), max(n, 1), _np_ptr(c),
                                                  max(n, 1), gemm_reps, b_chunks, t), "mmh_shard_sgemm_streamed")
            return c, dict(zip(("h2d", "bcast", "gemm", "d2h", "overlapped", "chunks", "first_pass", "wall"), list(t)))
        t = (C.c_float * 4)()
        _check(lib().mmh_shard_sgemm(self._h, m, n, k, _np_ptr(a), max(k, 1), _np_ptr(b), max(n, 1), _np_ptr(c),
                                     max(n, 1), gemm_reps, t), "mmh_shard_sgemm")
        return c, dict(zip(("h2d", "bcast", "gemm", "d2h"), list(t)))


def sgemm_sharded(ngpus: int, a: np.ndarray, b: np.ndarray, kernel="mfma"):
    """Single-process multi-device row-panel shard (mmh_sgemm_sharded).
    Returns (C, {"h2d","bcast","gemm","d2h"} ms)."""
    m, k = a.shape
    _, n = b.shape
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    c = np.zeros((m, n), dtype=np.float32)
    t = (C.c_float * 4)()
    _check(lib().mmh_sgemm_sharded(ngpus, m, n, k, _np_ptr(a), max(k, 1), _np_ptr(b), max(n, 1),
                                   _np_ptr(c), max(n, 1), _kernel_id(kernel), t), "mmh_sgemm_sharded")
    return c, dict(zip(("h2d", "bcast", "gemm", "d2h"), list(t)))


__all__ = ["MMult", "ShardedMMult", "MMultError", "lib", "use_ab_library", "device_count", "rccl_version", "shard_rows", "shard_chunks",
           "kernel_name", "last_launch", "use_timeline_library", "streamk_plan", "auto_plan", "igemm_plan", "auto_plan_op", "auto_plan_ex",
           "auto_plan_batched", "auto_plan_batched_ex", "sgemm_sharded", "BATCH_FORMS", "KERNELS", "CHAIN_KERNELS", "EXPORTS", "LIB_PATH",
           "AB_LIB_PATH", *_CONSTANTS]
