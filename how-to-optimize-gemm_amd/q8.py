"""The int8 linear layer (W8A8): libmmult_hip_q8.so behind torch tensors.

    from how_to_optimize_gemm_amd import q8
    qw = q8.QWeight(linear.weight.detach())            # once per layer: int8 image (transposed), one scale per output channel
    y = q8.qlinear(x, qw, bias, activation="relu")     # per call: one scale per row of x, int8 MFMA GEMM, fused epilogue
    layer = q8.QLinear.from_float(linear)              # the same as an inference-only torch.nn.Module

The binding is read from include/mmult_hip_q8.h (abi_header.parse); the numeric contract is in that header.  Everything runs
on torch's current stream; there is no CPU path and no backward.  torch is imported on first use, not with this module.
"""
from __future__ import annotations

import ctypes as C
import os

from . import abi_header as _abi
from . import api as _api
from .api import ACT_NONE, ACT_RELU, ERR_INVALID_ARG, ERR_UNSUPPORTED, OK, MMult, MMultError


class _OnDevice:
    """What MMult._tensor_args asks of its handle: the device ordinal."""

    def __init__(self, device: int):
        self.device = device


def tensor_args(t, rows, cols, what, dtype, device):
    """MMult._tensor_args -- the one statement of the tensor checks (dtype, device, unit column stride, rows that do not
    overlap) -- for a tensor that belongs to no handle: (data_ptr, leading dimension)."""
    return MMult._tensor_args(_OnDevice(device), t, rows, cols, what, dtype)

HEADER = os.path.join(os.path.dirname(_abi.HEADER), "mmult_hip_q8.h")
LIB_PATH = os.path.join(_api.PKG_DIR, "libmmult_hip_q8.so")
CONSTANTS, PROTOTYPES = _abi.parse(HEADER)
EXPORTS = list(PROTOTYPES)   # every symbol include/mmult_hip_q8.h declares
_STATUS_NAMES = {v: name for name, v in _abi.CONSTANTS.items() if name == "MMH_OK" or name.startswith("MMH_ERR_")}

_lib = None


def lib() -> C.CDLL:
    """Load libmmult_hip_q8.so (built in-tree by build.py) on the HIP runtime torch and libmmult_hip.so share.  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    _api._share_hip_runtime_with_torch()
    if not os.path.exists(LIB_PATH):
        raise MMultError(ERR_UNSUPPORTED, "load", f"{LIB_PATH} is missing -- run __graft_entry__.build(); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _check(status: int, where: str) -> None:
    if status != OK:
        last = lib().mmh_q8_last_error().decode()
        detail = _STATUS_NAMES.get(status, "unknown status")
        raise MMultError(status, where, f"{detail}; {last}" if last else detail)


def last_launch() -> str:
    """What the last qlinear / quantize_rows on this thread launched: the row quantiser's form and path, the GEMM's instantiation."""
    return lib().mmh_q8_last_launch().decode()


def _activation_id(activation, what: str) -> int:
    if activation not in (None, "relu"):
        raise MMultError(ERR_INVALID_ARG, what, "activation is None or 'relu'")
    return ACT_RELU if activation == "relu" else ACT_NONE


def qlinear_plan(rows: int, out_features: int, in_features: int, ldx: int = 0, ldy: int = 0, x_mod16: int = 0, y_mod16: int = 0,
                 bias: bool = False, activation=None, cu_count: int = 256):
    """(text, scratch bytes) of a qlinear call: what last_launch() says after it, and the bytes of the weight object's scratch
    it needs.  Host arithmetic only.  ldx / ldy 0: dense rows."""
    text, scratch = C.create_string_buffer(256), C.c_size_t(0)
    _check(lib().mmh_q8_linear_plan(rows, out_features, in_features, ldx or max(in_features, 1), ldy or out_features, x_mod16, y_mod16,
                                    int(bool(bias)), _activation_id(activation, "qlinear_plan"), cu_count, text, len(text),
                                    C.byref(scratch)), "mmh_q8_linear_plan")
    return text.value.decode(), scratch.value


class _DeviceArray:
    """Device memory of a QWeight as torch.as_tensor reads it (__cuda_array_interface__); keeps the owner alive."""

    def __init__(self, owner, ptr: int, shape, typestr: str):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 2}


def _stream(device: int) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream


class QWeight:
    """A layer's weight prepared once: `w` (out_features, in_features) fp32 on a GPU, torch's layout, read in place (any row
    stride).  Holds the int8 image transposed -- (in_features, pitch) with pitch = out_features rounded up to 16, pad columns
    0 --, one scale per output channel and the scales' reciprocals.  The preparation is enqueued on torch's current stream."""

    def __init__(self, w, device=None):
        import torch
        self._handle = None
        if w.dim() != 2:
            raise MMultError(ERR_INVALID_ARG, "QWeight", "need a 2-D weight (out_features, in_features)")
        self.device = w.device.index if device is None else int(device)
        self.out_features, self.in_features = int(w.shape[0]), int(w.shape[1])
        pw, ldw = tensor_args(w.detach(), self.out_features, self.in_features, "QWeight(w)", torch.float32, self.device)
        h = C.c_void_p()
        _check(lib().mmh_q8_weight_create(C.byref(h), self.device, self.out_features, self.in_features, pw, ldw, _stream(self.device)),
               "mmh_q8_weight_create")
        self._handle = h
        pitch, q, s, r = C.c_int(0), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().mmh_q8_weight_info(h, None, None, C.byref(pitch), C.byref(q), C.byref(s), C.byref(r)), "mmh_q8_weight_info")
        self.pitch = pitch.value
        self._ptrs = (q.value, s.value, r.value)

    def _view(self, ptr, shape, typestr):
        import torch
        if 0 in shape:
            return torch.empty(shape, dtype=torch.int8 if typestr == "|i1" else torch.float32, device=f"cuda:{self.device}")
        return torch.as_tensor(_DeviceArray(self, ptr, shape, typestr), device=f"cuda:{self.device}")

    @property
    def q(self):
        """The int8 image, (in_features, pitch): q[k, j] = Q(w[j, :])[k].  A view of the object's memory."""
        return self._view(self._ptrs[0], (self.in_features, self.pitch), "|i1")

    @property
    def scale(self):
        """(out_features,) fp32: 127 / max|w[j, :]|."""
        return self._view(self._ptrs[1], (self.out_features,), "<f4")

    @property
    def inv_scale(self):
        """(out_features,) fp32: fl(1 / scale)."""
        return self._view(self._ptrs[2], (self.out_features,), "<f4")

    def reserve(self, max_rows: int) -> None:
        """Size the object's scratch for calls of up to max_rows rows (before capturing a graph of larger calls than were run)."""
        _check(lib().mmh_q8_linear_reserve(self._handle, int(max_rows), _stream(self.device)), "mmh_q8_linear_reserve")

    def close(self) -> None:
        if self._handle is not None:
            lib().mmh_q8_weight_destroy(self._handle)
            self._handle = None

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass


def quantize_rows(x, out=None):
    """(q, scale, inv_scale) of a 2-D fp32 GPU tensor, one scale per row: q int8 like x, scale = 127 / max|row|, inv_scale =
    fl(1 / scale).  `out`: an int8 (rows, cols) window to write (any row stride; up to 15 bytes behind each row, inside the
    stride, are zeroed); default: rows of pitch cols rounded up to 16."""
    import torch
    if x.dim() != 2:
        raise MMultError(ERR_INVALID_ARG, "quantize_rows", "need a 2-D tensor")
    rows, cols = x.shape
    device = x.device.index
    px, ldx = tensor_args(x, rows, cols, "quantize_rows(x)", torch.float32, device)
    if out is None:
        pitch = (cols + 15) & ~15
        base = torch.empty((rows, pitch), dtype=torch.int8, device=x.device)
        out, pq, ldq = base[:, :cols], base.data_ptr(), max(pitch, 1)
    else:
        pq, ldq = tensor_args(out, rows, cols, "quantize_rows(out)", torch.int8, device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    inv_scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    _check(lib().mmh_q8_quantize_rows(device, rows, cols, px, ldx, pq, ldq, scale.data_ptr(), inv_scale.data_ptr(), _stream(device)),
           "mmh_q8_quantize_rows")
    return out, scale, inv_scale


def _linear_args(what, x, qweight, bias, activation, out):
    """mmh_q8_linear's arguments between the object and the stream, and `out`."""
    import torch
    act = _activation_id(activation, what)
    if x.dim() != 2 or x.shape[1] != qweight.in_features:
        raise MMultError(ERR_INVALID_ARG, what, f"need a 2-D x (rows, {qweight.in_features})")
    if x.requires_grad:
        raise MMultError(ERR_INVALID_ARG, what, "the int8 layer has no backward: x requires grad")
    rows, dev = x.shape[0], qweight.device
    if out is None:
        out = torch.empty((rows, qweight.out_features), dtype=torch.float32, device=x.device)
    px, ldx = tensor_args(x, rows, qweight.in_features, what + "(x)", torch.float32, dev)
    py, ldy = tensor_args(out, rows, qweight.out_features, what + "(out)", torch.float32, dev)
    pbias = None
    if bias is not None:
        if not bias.is_cuda or bias.device.index != dev or bias.dtype != torch.float32 or bias.dim() != 1 or \
                bias.shape[0] != qweight.out_features or (bias.shape[0] > 1 and bias.stride(0) != 1):
            raise MMultError(ERR_INVALID_ARG, what, "the bias is a dense 1-D fp32 tensor on the weight's device, one float per output column")
        pbias = bias.data_ptr()
    return (rows, px, ldx, pbias, act, py, ldy), out


def qlinear(x, qweight: QWeight, bias=None, activation=None, out=None):
    """y = act(x @ w.t() + bias) in int8 (the header's contract): x (rows, in_features) fp32, quantised per row on the way in;
    bias (out_features,) or None; activation None or "relu"; `out` (rows, out_features) fp32, any row stride."""
    args, out = _linear_args("qlinear", x, qweight, bias, activation, out)
    if args[0] > 0:
        _check(lib().mmh_q8_linear(qweight._handle, *args, _stream(qweight.device)), "mmh_q8_linear")
    return out


def time_qlinear(x, qweight: QWeight, bias=None, activation=None, out=None, warmup: int = 1, reps: int = 20) -> float:
    """Mean milliseconds per qlinear call (one event pair around `reps` calls)."""
    args, _ = _linear_args("time_qlinear", x, qweight, bias, activation, out)
    ms = C.c_float(0.0)
    _check(lib().mmh_time_q8_linear(qweight._handle, *args, warmup, reps, _stream(qweight.device), C.byref(ms)), "mmh_time_q8_linear")
    return ms.value


def _make_qlinear_class():
    import torch

    class QLinear(torch.nn.Module):
        """torch.nn.Linear (+ ReLU) in int8, inference only: the weight is a QWeight (set_weight / from_float), the bias an
        fp32 buffer.  forward flattens leading dimensions to rows; an input that requires grad raises."""

        def __init__(self, in_features: int, out_features: int, bias: bool = True, activation=None):
            super().__init__()
            _activation_id(activation, "QLinear")
            self.in_features, self.out_features, self.activation = in_features, out_features, activation
            self.qweight = None
            self.register_buffer("bias", torch.zeros(out_features) if bias else None)

        def set_weight(self, w, bias=None):
            """Prepare `w` (out_features, in_features) fp32 on a GPU; `bias` replaces the bias buffer's values."""
            if tuple(w.shape) != (self.out_features, self.in_features):
                raise MMultError(ERR_INVALID_ARG, "QLinear.set_weight", f"need a ({self.out_features},{self.in_features}) weight")
            self.qweight = QWeight(w)
            if self.bias is not None:
                self.bias = (torch.zeros(self.out_features) if bias is None else bias.detach().to(torch.float32)).to(w.device).contiguous()
            return self

        @classmethod
        def from_float(cls, linear, activation=None):
            """The int8 layer of a torch.nn.Linear whose weight lives on a GPU."""
            return cls(linear.in_features, linear.out_features, linear.bias is not None, activation).set_weight(
                linear.weight.detach(), None if linear.bias is None else linear.bias.detach())

        def forward(self, x):
            if self.qweight is None:
                raise MMultError(ERR_INVALID_ARG, "QLinear", "no weight prepared: set_weight() or from_float() first")
            if x.requires_grad:
                raise MMultError(ERR_INVALID_ARG, "QLinear", "the int8 layer has no backward: x requires grad")
            rows = x.reshape(-1, self.in_features)
            if rows.shape[0] > 1 and rows.shape[1] > 1 and rows.stride(1) != 1:
                rows = rows.contiguous()
            y = qlinear(rows, self.qweight, self.bias, self.activation)
            return y.reshape(*x.shape[:-1], self.out_features)

        def extra_repr(self) -> str:
            return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, activation={self.activation}"

    return QLinear


def __getattr__(name):   # QLinear is a torch.nn.Module: made when first asked for, so that importing this module does not import torch
    if name == "QLinear":
        cls = globals()["QLinear"] = _make_qlinear_class()
        return cls
    raise AttributeError(name)


__all__ = ["QWeight", "QLinear", "quantize_rows", "qlinear", "time_qlinear", "qlinear_plan", "last_launch", "lib", "EXPORTS", "LIB_PATH", "HEADER"]
