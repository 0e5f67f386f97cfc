"""The int8 linear layer (W8A8): libmmult_hip_q8.so behind torch tensors.

    from how_to_optimize_gemm_amd import q8
    qw = q8.QWeight(linear.weight.detach())            # once per layer: int8 image (transposed), one scale per output channel
    y = q8.qlinear(x, qw, bias, activation="relu")     # per call: one scale per row of x, int8 MFMA GEMM, fused epilogue
    layer = q8.QLinear.from_float(linear)              # the same as an inference-only torch.nn.Module
    xq = q8.quantize(x)                                # a QRows: one quantisation for any number of weights (Q/K/V, gate/up)
    y = q8.qlinear(xq, qw, bias)                       # ... straight into the GEMM: no quantiser pass
    hq = q8.qlinear(xq, qw, bias, "relu", out_scale=s) # int8 out (libmmult_hip_q8o.so): the next layer's QRows, no fp32 round trip
    mlp = q8.QMLP.from_float([fc1, fc2]); mlp.calibrate(x); y = mlp(x)    # one quantiser, int8 -> int8 hidden layers, fp32 out
    y = q8.qlinear_decode(xq, qw, bias)                # 1 - 16 rows (libmmult_hip_q8d.so): split-K strips, the same bits as qlinear
    qw4 = q8.QWeight4(linear.weight.detach())          # 4-bit weights (W4A8, libmmult_hip_q4d.so): packed nibbles, half the bytes
    y = q8.qlinear_decode(xq, qw4, bias)               # ... for 1 - 16 rows only: there are no 4-bit tiles
    qw4g = q8.QWeight4G(linear.weight.detach())        # ... with one scale per group of 128 input features (libmmult_hip_q4g.so):
    y = q8.qlinear_decode(xq, qw4g, bias, splits=4)    # its own bit contract, which depends on the K partition -- force it to pin the bits
    mlp4 = q8.QMLP([qw4a, qw4b], biases, decode=True)  # a stack may hold QWeight4s (mixed with QWeights) with decode=True only:
                                                       # calibrate / forward take 1 - 16 rows, more raise ERR_UNSUPPORTED

The binding is read from include/mmult_hip_q8.h (abi_header.parse); the numeric contract is in that header.  The int8-output
library is loaded on first use, its binding read from include/mmult_hip_q8o.h.  Everything runs
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

_STATUS_NAMES = {v: name for name, v in _abi.CONSTANTS.items() if name == "MMH_OK" or name.startswith("MMH_ERR_")}


class _Library:
    """One of the layer's libraries (built in-tree by build.py): `header` under include/ is parsed now, `path` is loaded on
    first use, on the HIP runtime torch and libmmult_hip.so share, and every prototype of the header is bound.  `prefix` names
    its <prefix>_last_error and <prefix>_last_launch.  Fails loudly."""

    def __init__(self, header: str, path: str, prefix: str):
        self.header = os.path.join(os.path.dirname(_abi.HEADER), header)
        self.path = os.path.join(_api.PKG_DIR, path)
        self.prefix = prefix
        self.constants, self.prototypes = _abi.parse(self.header)
        self._lib = None

    def lib(self) -> C.CDLL:
        if self._lib is None:
            _api._share_hip_runtime_with_torch()
            if not os.path.exists(self.path):
                raise MMultError(ERR_UNSUPPORTED, "load", f"{self.path} is missing -- run __graft_entry__.build(); there is no CPU fallback")
            L = C.CDLL(self.path)
            for name, (restype, argtypes) in self.prototypes.items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
            self._lib = L
        return self._lib

    def check(self, status: int, where: str) -> None:
        if status != OK:
            last = getattr(self.lib(), self.prefix + "_last_error")().decode()
            detail = _STATUS_NAMES.get(status, "unknown status")
            raise MMultError(status, where, f"{detail}; {last}" if last else detail)

    def last_launch(self) -> str:
        return getattr(self.lib(), self.prefix + "_last_launch")().decode()


_q8 = _Library("mmult_hip_q8.h", "libmmult_hip_q8.so", "mmh_q8")       # fp32 out, the weight object, the row quantiser
_q8o = _Library("mmult_hip_q8o.h", "libmmult_hip_q8o.so", "mmh_q8o")   # int8 out
_q8d = _Library("mmult_hip_q8d.h", "libmmult_hip_q8d.so", "mmh_q8d")   # 1 - 16 rows, split-K
_q4d = _Library("mmult_hip_q4d.h", "libmmult_hip_q4d.so", "mmh_q4d")   # 1 - 16 rows on packed 4-bit weights
_q4g = _Library("mmult_hip_q4g.h", "libmmult_hip_q4g.so", "mmh_q4g")   # ... with one scale per group of 128 input features
HEADER, LIB_PATH, CONSTANTS, PROTOTYPES = _q8.header, _q8.path, _q8.constants, _q8.prototypes
EXPORTS = list(PROTOTYPES)   # every symbol include/mmult_hip_q8.h declares
Q8O_HEADER, Q8O_LIB_PATH = _q8o.header, _q8o.path
Q8D_HEADER, Q8D_LIB_PATH = _q8d.header, _q8d.path
Q4D_HEADER, Q4D_LIB_PATH = _q4d.header, _q4d.path
Q4G_HEADER, Q4G_LIB_PATH = _q4g.header, _q4g.path
Q8D_MAX_ROWS = _q8d.constants["MMH_Q8D_MAX_ROWS"]
Q4D_MAX_ROWS = _q4d.constants["MMH_Q4D_MAX_ROWS"]
Q4G_GROUP = _q4g.constants["MMH_Q4G_GROUP"]
lib, lib_q8o, lib_q8d, lib_q4d, lib_q4g = _q8.lib, _q8o.lib, _q8d.lib, _q4d.lib, _q4g.lib   # the loaded ctypes libraries
_check = _q8.check


def last_launch() -> str:
    """What the last qlinear / quantize_rows on this thread launched: the row quantiser's form and path, the GEMM's instantiation."""
    return _q8.last_launch()


def last_launch_q8o() -> str:
    """What the last int8-output qlinear on this thread launched."""
    return _q8o.last_launch()


def last_launch_q8d() -> str:
    """What the last qlinear_decode on this thread launched."""
    return _q8d.last_launch()


def last_launch_q4d() -> str:
    """What the last qlinear_decode on a QWeight4 on this thread launched."""
    return _q4d.last_launch()


def last_launch_q4g() -> str:
    """What the last qlinear_decode on a QWeight4G on this thread launched."""
    return _q4g.last_launch()


def qlinear_s8o_plan(rows: int, out_features: int, in_features: int, ldq: int = 0, pitch_n: int = 0, ldyq: int = 0, xq_mod4: int = 0,
                     wq_mod4: int = 0, yq_mod4: int = 0, cu_count: int = 256) -> str:
    """The launch text of an int8-output qlinear call.  Host arithmetic only.  ldq / pitch_n / ldyq 0: rows of the default
    pitch (the length rounded up to 16)."""
    p16 = lambda n: (n + 15) & ~15
    text = C.create_string_buffer(128)
    _q8o.check(lib_q8o().mmh_q8o_linear_plan(rows, out_features, in_features, ldq or p16(in_features), pitch_n or p16(out_features),
                                             ldyq or p16(out_features), xq_mod4, wq_mod4, yq_mod4, cu_count, text, len(text)),
               "mmh_q8o_linear_plan")
    return text.value.decode()


def qlinear_decode_plan(rows: int, out_features: int, in_features: int, ldq: int = 0, pitch_n: int = 0, out8: bool = False, ldo: int = 0,
                        xq_mod4: int = 0, wq_mod4: int = 0, o_mod16: int = 0, splits: int = 0, cu_count: int = 256):
    """(text, work bytes) of a qlinear_decode call: what last_launch_q8d() says after it and the workspace it needs.  Host
    arithmetic only.  ldq / pitch_n 0: rows of the default pitch (the length rounded up to 16); ldo 0: dense fp32 rows, int8
    rows of the default pitch."""
    p16 = lambda n: (n + 15) & ~15
    text, work = C.create_string_buffer(192), C.c_size_t(0)
    _q8d.check(lib_q8d().mmh_q8d_linear_plan(rows, out_features, in_features, ldq or p16(in_features), pitch_n or p16(out_features),
                                             int(bool(out8)), ldo or (p16(out_features) if out8 else out_features), xq_mod4, wq_mod4,
                                             o_mod16, splits, cu_count, text, len(text), C.byref(work)), "mmh_q8d_linear_plan")
    return text.value.decode(), work.value


def qlinear_decode4_plan(rows: int, out_features: int, in_features: int, ldq: int = 0, pitch_n: int = 0, out8: bool = False, ldo: int = 0,
                         xq_mod4: int = 0, wp_mod4: int = 0, o_mod16: int = 0, splits: int = 0, cu_count: int = 256):
    """qlinear_decode_plan for a QWeight4: (text, work bytes) of the call, what last_launch_q4d() says after it.  The same
    arguments and defaults; pitch_n is the packed image's."""
    p16 = lambda n: (n + 15) & ~15
    text, work = C.create_string_buffer(192), C.c_size_t(0)
    _q4d.check(lib_q4d().mmh_q4d_linear_plan(rows, out_features, in_features, ldq or p16(in_features), pitch_n or p16(out_features),
                                             int(bool(out8)), ldo or (p16(out_features) if out8 else out_features), xq_mod4, wp_mod4,
                                             o_mod16, splits, cu_count, text, len(text), C.byref(work)), "mmh_q4d_linear_plan")
    return text.value.decode(), work.value


def qlinear_decode4g_plan(rows: int, out_features: int, in_features: int, ldq: int = 0, pitch_n: int = 0, out8: bool = False, ldo: int = 0,
                          xq_mod4: int = 0, wp_mod4: int = 0, o_mod16: int = 0, splits: int = 0, cu_count: int = 256, pitch_s: int = 0,
                          gs_mod16: int = 0):
    """qlinear_decode_plan for a QWeight4G: (text, work bytes) of the call, what last_launch_q4g() says after it -- the K
    partition its bits depend on.  The same arguments and defaults; pitch_n is the packed image's, pitch_s the group scales'
    (0: out_features rounded up to 16), gs_mod16 their base modulo 16."""
    p16 = lambda n: (n + 15) & ~15
    text, work = C.create_string_buffer(192), C.c_size_t(0)
    _q4g.check(lib_q4g().mmh_q4g_linear_plan(rows, out_features, in_features, ldq or p16(in_features), pitch_n or p16(out_features),
                                             pitch_s or p16(out_features), int(bool(out8)),
                                             ldo or (p16(out_features) if out8 else out_features), xq_mod4, wp_mod4, gs_mod16, o_mod16,
                                             splits, cu_count, text, len(text), C.byref(work)), "mmh_q4g_linear_plan")
    return text.value.decode(), work.value


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


class _DecodeWork:
    """qlinear_decode's split-K partials of a prepared weight: a torch uint8 tensor cached on the weight, grown outside capture
    only.  The weight says what a call needs through _decode_plan (its library's plan)."""

    _decode_work = None
    _decode_plan = staticmethod(qlinear_decode_plan)

    def _decode_workspace(self, nbytes: int):
        """The cached workspace of qlinear_decode, at least nbytes long (torch's allocations are 16-byte aligned)."""
        import torch
        if self._decode_work is None or self._decode_work.numel() < nbytes:
            if torch.cuda.is_current_stream_capturing():
                raise MMultError(ERR_UNSUPPORTED, "qlinear_decode", "the workspace would have to grow while the stream is capturing -- "
                                 f"call {type(self).__name__}.reserve_decode() first")
            self._decode_work = torch.empty((max(int(nbytes), 16),), dtype=torch.uint8, device=f"cuda:{self.device}")
        return self._decode_work

    def reserve_decode(self, splits: int = 0) -> None:
        """Size qlinear_decode's workspace for every call of 1 - 16 rows on this weight (before capturing a graph): the plan's
        own split count, or a forced one."""
        if self.in_features == 0 or self.out_features == 0:
            return
        cus = _cu_count(self.device)
        self._decode_workspace(max(self._decode_plan(rows, self.out_features, self.in_features, pitch_n=self.pitch, splits=splits,
                                                     cu_count=cus)[1] for rows in range(1, Q8D_MAX_ROWS + 1)))


class QWeight(_DecodeWork):
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
        self._decode_work = None   # qlinear_decode's split-K partials: a torch uint8 tensor, grown outside capture

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
        self._decode_work = None
        if self._handle is not None:
            lib().mmh_q8_weight_destroy(self._handle)
            self._handle = None

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass


class QWeight4(_DecodeWork):
    """A layer's weight at FOUR bits per element (W4A8), prepared once: `w` (out_features, in_features) fp32 on a GPU, torch's
    layout, read in place (any row stride).  Owns three torch tensors: `p`, the packed uint8 image (packed_rows, pitch) -- pitch =
    out_features rounded up to 16, 64 rows per 128 input features, a byte's low nibble the first half of its slice and its high
    nibble the second (include/mmult_hip_q4d.h has the layout) --, `scale` (out_features,) = 7 / max|w[j, :]| and `inv_scale` =
    fl(1 / scale).  Read by qlinear_decode only: 1 - 16 rows.  The preparation is enqueued on torch's current stream."""

    _decode_plan = staticmethod(qlinear_decode4_plan)

    def __init__(self, w, device=None):
        import torch
        if w.dim() != 2:
            raise MMultError(ERR_INVALID_ARG, "QWeight4", "need a 2-D weight (out_features, in_features)")
        self.device = w.device.index if device is None else int(device)
        self.out_features, self.in_features = int(w.shape[0]), int(w.shape[1])
        pw, ldw = tensor_args(w.detach(), self.out_features, self.in_features, "QWeight4(w)", torch.float32, self.device)
        self.pitch, packed_rows, _ = weight4_layout(self.out_features, self.in_features)
        dev = f"cuda:{self.device}"
        self.p = torch.empty((packed_rows, self.pitch), dtype=torch.uint8, device=dev)
        self.scale = torch.empty((self.out_features,), dtype=torch.float32, device=dev)
        self.inv_scale = torch.empty((self.out_features,), dtype=torch.float32, device=dev)
        _q4d.check(lib_q4d().mmh_q4d_pack_weight(self.device, self.out_features, self.in_features, pw, ldw, self.p.data_ptr(), self.pitch,
                                                 self.scale.data_ptr(), self.inv_scale.data_ptr(), _stream(self.device)), "mmh_q4d_pack_weight")

    @classmethod
    def _adopt_image(cls, p, out_features: int, in_features: int):
        """from_image's first half: a new object that holds the caller's packed image `p`, its device and its pitch."""
        import torch
        self = cls.__new__(cls)
        self.out_features, self.in_features = int(out_features), int(in_features)
        packed_rows = weight4_layout(self.out_features, self.in_features)[1]
        if not (torch.is_tensor(p) and p.is_cuda and p.dtype == torch.uint8 and p.dim() == 2 and p.shape[0] == packed_rows
                and p.shape[1] >= self.out_features):
            raise MMultError(ERR_INVALID_ARG, cls.__name__ + ".from_image", f"p is a ({packed_rows}, >= {self.out_features}) uint8 tensor on a GPU")
        self.device = p.device.index
        self.pitch = int(p.shape[1])
        if packed_rows:
            _, self.pitch = tensor_args(p, packed_rows, int(p.shape[1]), cls.__name__ + ".from_image(p)", torch.uint8, self.device)
            if self.pitch % 4 or p.data_ptr() % 4:
                raise MMultError(ERR_INVALID_ARG, cls.__name__ + ".from_image", "the kernel reads p in dwords: a row stride that is a multiple "
                                 "of 4 and a 4-byte aligned base")
        self.p = p
        return self

    @classmethod
    def from_image(cls, p, inv_scale, out_features: int, in_features: int):
        """Adopt a caller-made packed image: `p` uint8 (64 * ceil(in_features / 128), pitch >= out_features) on a GPU with unit
        column stride, a row stride that is a multiple of 4 and a 4-byte aligned base, every nibble of an input feature >=
        in_features zero (-8 is allowed); `inv_scale` a dense (out_features,) fp32 tensor, one factor per output channel.  `scale`
        is None."""
        import torch
        self = cls._adopt_image(p, out_features, in_features)
        if not (torch.is_tensor(inv_scale) and inv_scale.is_cuda and inv_scale.device.index == self.device and inv_scale.dtype == torch.float32
                and inv_scale.dim() == 1 and inv_scale.shape[0] == self.out_features and (self.out_features <= 1 or inv_scale.stride(0) == 1)):
            raise MMultError(ERR_INVALID_ARG, "QWeight4.from_image", "inv_scale is a dense (out_features,) fp32 tensor on p's device")
        self.p, self.scale, self.inv_scale = p, None, inv_scale
        return self

    @property
    def _ptrs(self):
        """(image, scale, inv_scale) addresses, as QWeight's."""
        return (self.p.data_ptr() if self.p.numel() else None, None if self.scale is None else self.scale.data_ptr(), self.inv_scale.data_ptr())

    @property
    def nbytes(self) -> int:
        """The packed image's bytes."""
        return int(self.p.shape[0]) * self.pitch

    def unpack(self):
        """The int8 image QWeight.q would be, (in_features, pitch): values in -8 .. 7.  torch ops on the packed tensor."""
        import torch
        slices = self.p.shape[0] // 64
        p = self.p.view(slices, 64, self.p.shape[1]).to(torch.int16)
        lo, hi = p & 15, p >> 4
        w = torch.stack([lo, hi], 1).reshape(slices * 128, self.p.shape[1])
        return torch.where(w >= 8, w - 16, w).to(torch.int8)[:self.in_features]

    def close(self) -> None:
        self._decode_work = None


class QWeight4G(QWeight4):
    """A QWeight4 with ONE SCALE PER GROUP of 128 consecutive input features of every output channel (GPTQ / AWQ style), prepared
    once from `w` (out_features, in_features) fp32 on a GPU.  Owns `p`, QWeight4's packed image byte for byte in layout, and
    `group_scale` / `group_inv_scale`, fp32 (groups, pitch_s) with groups = ceil(in_features / 128) and pitch_s = out_features
    rounded up to 16 (pad columns 0): 7 / max|w[j, 128 g : 128 g + 128]| and its reciprocal.  `scale` and `inv_scale` are None.
    Read by qlinear_decode only, 1 - 16 rows, under include/mmult_hip_q4g.h's contract."""

    _decode_plan = staticmethod(qlinear_decode4g_plan)

    def __init__(self, w, group_size: int = 128, device=None):
        import torch
        if group_size != Q4G_GROUP:
            raise MMultError(ERR_INVALID_ARG, "QWeight4G", f"group_size is {Q4G_GROUP}: a group is one slice of the packed image")
        if w.dim() != 2:
            raise MMultError(ERR_INVALID_ARG, "QWeight4G", "need a 2-D weight (out_features, in_features)")
        self.group_size = Q4G_GROUP
        self.device = w.device.index if device is None else int(device)
        self.out_features, self.in_features = int(w.shape[0]), int(w.shape[1])
        pw, ldw = tensor_args(w.detach(), self.out_features, self.in_features, "QWeight4G(w)", torch.float32, self.device)
        self.pitch, packed_rows, groups, self.pitch_s, _, _ = weight4g_layout(self.out_features, self.in_features)
        dev = f"cuda:{self.device}"
        self.p = torch.empty((packed_rows, self.pitch), dtype=torch.uint8, device=dev)
        self.group_scale = torch.empty((groups, self.pitch_s), dtype=torch.float32, device=dev)
        self.group_inv_scale = torch.empty((groups, self.pitch_s), dtype=torch.float32, device=dev)
        self.scale = self.inv_scale = None
        _q4g.check(lib_q4g().mmh_q4g_pack_weight(self.device, self.out_features, self.in_features, pw, ldw, self.p.data_ptr(), self.pitch,
                                                 self.group_scale.data_ptr(), self.group_inv_scale.data_ptr(), self.pitch_s,
                                                 _stream(self.device)), "mmh_q4g_pack_weight")

    @classmethod
    def from_image(cls, p, group_inv_scale, out_features: int, in_features: int):
        """Adopt caller-made operands: `p` as QWeight4.from_image takes it; `group_inv_scale` an fp32 (ceil(in_features / 128),
        >= out_features) tensor on p's device with unit column stride, a row stride that is a multiple of 4 floats and a 16-byte
        aligned base (the kernel reads four factors as one vector), one factor per group and output channel.  `group_scale` is None."""
        import torch
        self = cls._adopt_image(p, out_features, in_features)
        groups = -(-self.in_features // Q4G_GROUP)
        g = group_inv_scale
        if not (torch.is_tensor(g) and g.is_cuda and g.device.index == self.device and g.dtype == torch.float32 and g.dim() == 2
                and g.shape[0] == groups and g.shape[1] >= self.out_features):
            raise MMultError(ERR_INVALID_ARG, "QWeight4G.from_image", f"group_inv_scale is a ({groups}, >= {self.out_features}) fp32 tensor on p's device")
        self.pitch_s = int(g.shape[1])
        if groups:
            _, self.pitch_s = tensor_args(g, groups, int(g.shape[1]), "QWeight4G.from_image(group_inv_scale)", torch.float32, self.device)
            if groups == 1 and g.stride(0) >= g.shape[1]:
                self.pitch_s = int(g.stride(0))
            if self.pitch_s % 4 or g.data_ptr() % 16:
                raise MMultError(ERR_INVALID_ARG, "QWeight4G.from_image", "the kernel reads four group scales as one vector: a row stride that "
                                 "is a multiple of 4 floats and a 16-byte aligned base")
        self.group_size = Q4G_GROUP
        self.scale = self.inv_scale = self.group_scale = None
        self.group_inv_scale = g
        return self

    @property
    def _ptrs(self):
        """(image, None, group_inv_scale) addresses, as QWeight4's."""
        return (self.p.data_ptr() if self.p.numel() else None, None, self.group_inv_scale.data_ptr() if self.group_inv_scale.numel() else None)

    @property
    def nbytes(self) -> int:
        """The packed image's bytes plus the group scales' (the reciprocals: what the layer reads)."""
        return int(self.p.shape[0]) * self.pitch + int(self.group_inv_scale.shape[0]) * self.pitch_s * 4

    def dequantize(self):
        """The fp32 (out_features, in_features) weight the layer multiplies by: unpack() times the groups' factors.  torch ops."""
        import torch
        n, k = self.out_features, self.in_features
        r = self.group_inv_scale[:, :n].repeat_interleave(Q4G_GROUP, dim=0)[:k]
        return (self.unpack()[:, :n].to(torch.float32) * r).t().contiguous()


def weight4g_layout(out_features: int, in_features: int):
    """(pitch, packed rows, groups, pitch_s, image bytes, scale bytes) of the library's own grouped 4-bit layout.  Host arithmetic only."""
    pitch, rows, groups, pitch_s, image, scales = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0), C.c_size_t(0)
    _q4g.check(lib_q4g().mmh_q4g_weight_layout(int(out_features), int(in_features), C.byref(pitch), C.byref(rows), C.byref(groups),
                                               C.byref(pitch_s), C.byref(image), C.byref(scales)), "mmh_q4g_weight_layout")
    return pitch.value, rows.value, groups.value, pitch_s.value, image.value, scales.value


def weight4_layout(out_features: int, in_features: int):
    """(pitch, packed rows, bytes) of the library's own packed 4-bit image.  Host arithmetic only."""
    pitch, rows, nbytes = C.c_int(0), C.c_int(0), C.c_size_t(0)
    _q4d.check(lib_q4d().mmh_q4d_weight_layout(int(out_features), int(in_features), C.byref(pitch), C.byref(rows), C.byref(nbytes)),
               "mmh_q4d_weight_layout")
    return pitch.value, rows.value, nbytes.value


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


class QRows:
    """A quantised activation: `q` (rows, cols) int8 on a GPU -- unit column stride, a row stride that is a multiple of 4, a
    4-byte aligned base: what the GEMM's tile reads in place --, and `inv_scale` (rows,) fp32, the reciprocal of each row's
    scale (the contract's rx).  What quantize() and an int8-output qlinear return and what qlinear takes as x."""

    def __init__(self, q, inv_scale):
        import torch
        if not (torch.is_tensor(q) and q.dim() == 2):
            raise MMultError(ERR_INVALID_ARG, "QRows", "q is a 2-D int8 tensor")
        self.rows, self.cols = int(q.shape[0]), int(q.shape[1])
        self.device = q.device.index
        if self.cols == 0:   # (nothing is read: any int8 tensor of that shape on a GPU)
            if not q.is_cuda or q.dtype != torch.int8:
                raise MMultError(ERR_INVALID_ARG, "QRows", "q is a 2-D int8 tensor on a GPU")
            ptr, ld = None, 0
        else:
            ptr, ld = tensor_args(q, self.rows, self.cols, "QRows(q)", torch.int8, self.device)
            if self.rows <= 1:   # (one row has no row stride to go by: its view's, where that holds the row, else the row's length)
                ld = q.stride(0) if self.rows == 1 and q.stride(0) >= self.cols and q.stride(0) % 4 == 0 else (self.cols + 3) & ~3
            if ld % 4 or ptr % 4:
                raise MMultError(ERR_INVALID_ARG, "QRows", "the GEMM reads q in dwords: a row stride that is a multiple of 4 and a 4-byte aligned base")
        if not (torch.is_tensor(inv_scale) and inv_scale.is_cuda and inv_scale.device.index == self.device and inv_scale.dtype == torch.float32
                and inv_scale.dim() == 1 and inv_scale.shape[0] == self.rows and (self.rows <= 1 or inv_scale.stride(0) == 1)):
            raise MMultError(ERR_INVALID_ARG, "QRows", "inv_scale is a dense (rows,) fp32 tensor on q's device")
        self.q, self.inv_scale, self._ptr, self._ld = q, inv_scale, ptr, ld

    @classmethod
    def _of_window(cls, q, inv_scale, ptr, ld):
        """What an int8-output qlinear wrote into a caller's window: any pitch, any base.  Whether the GEMM can read it in place
        is asked when it is used as x (_rows_args)."""
        self = cls.__new__(cls)
        self.rows, self.cols, self.device = int(q.shape[0]), int(q.shape[1]), q.device.index
        self.q, self.inv_scale, self._ptr, self._ld = q, inv_scale, ptr, ld
        return self


def quantize(x) -> QRows:
    """quantize_rows(x) with its default pitch, as the QRows qlinear reads."""
    q, _, inv_scale = quantize_rows(x)
    return QRows(q, inv_scale)


def _bias_ptr(what, bias, qweight):
    import torch
    if bias is None:
        return None
    if not bias.is_cuda or bias.device.index != qweight.device or bias.dtype != torch.float32 or bias.dim() != 1 or \
            bias.shape[0] != qweight.out_features or (bias.shape[0] > 1 and bias.stride(0) != 1):
        raise MMultError(ERR_INVALID_ARG, what, "the bias is a dense 1-D fp32 tensor on the weight's device, one float per output column")
    return bias.data_ptr()


def _float_rows(what, x, qweight) -> None:
    """What every entry point asks of an fp32 x: (rows, in_features), and no gradient to lose."""
    if x.dim() != 2 or x.shape[1] != qweight.in_features:
        raise MMultError(ERR_INVALID_ARG, what, f"need a 2-D x (rows, {qweight.in_features})")
    if x.requires_grad:
        raise MMultError(ERR_INVALID_ARG, what, "the int8 layer has no backward: x requires grad")


def _rows_args(what, x: QRows, qweight):
    if x.cols != qweight.in_features or x.device != qweight.device:
        raise MMultError(ERR_INVALID_ARG, what, f"need QRows of {qweight.in_features} columns on the weight's device")
    if x.cols and (x._ld % 4 or x._ptr % 4):
        raise MMultError(ERR_INVALID_ARG, what, "the GEMM reads x.q in dwords: a row stride that is a multiple of 4 and a 4-byte aligned base")
    return x.rows, x._ptr, x._ld, x.inv_scale.data_ptr()


def _linear_s8_args(what, x: QRows, qweight, bias, activation, out):
    """mmh_q8_linear_s8's arguments between the object and the stream, and `out`."""
    import torch
    act = _activation_id(activation, what)
    rows, pxq, ldq, prx = _rows_args(what, x, qweight)
    if out is None:
        out = torch.empty((rows, qweight.out_features), dtype=torch.float32, device=x.q.device)
    py, ldy = tensor_args(out, rows, qweight.out_features, what + "(out)", torch.float32, qweight.device)
    return (rows, pxq, ldq, prx, _bias_ptr(what, bias, qweight), act, py, ldy), out


def _scale_vectors(what, out_scale, rows, device):
    """(so, fl(1 / so)): two (rows,) fp32 device tensors of an out_scale given as a Python float or as such a tensor."""
    import numpy as np
    import torch
    if torch.is_tensor(out_scale):
        if not (out_scale.is_cuda and out_scale.device.index == device and out_scale.dtype == torch.float32 and out_scale.dim() == 1
                and out_scale.shape[0] == rows and (rows <= 1 or out_scale.stride(0) == 1)):
            raise MMultError(ERR_INVALID_ARG, what, "out_scale is a Python float or a dense (rows,) fp32 tensor on the weight's device")
        # the double quotient rounded to float IS the float quotient (53 >= 2 * 24 + 2 bits: the second rounding is innocuous)
        return out_scale, (1.0 / out_scale.double()).float()
    so = np.float32(out_scale)
    if not np.isfinite(so):
        raise MMultError(ERR_INVALID_ARG, what, "out_scale must be finite")
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / so
    dev = f"cuda:{device}"
    return torch.full((rows,), float(so), dtype=torch.float32, device=dev), torch.full((rows,), float(inv), dtype=torch.float32, device=dev)


def _out_window(what, out, rows, n, out8, device):
    """(out, address, leading dimension) of a (rows, n) result on `device`: the caller's `out`, or new rows -- int8 (out8) of
    pitch n rounded up to 16, else dense fp32.  One row has no row stride to go by: its view's, where that holds the row."""
    import torch
    dtype = torch.int8 if out8 else torch.float32
    if out is None:
        out = torch.empty((rows, (n + 15) & ~15), dtype=dtype, device=f"cuda:{device}")[:, :n] if out8 else \
            torch.empty((rows, n), dtype=dtype, device=f"cuda:{device}")
    po, ldo = tensor_args(out, rows, n, what + "(out)", dtype, device)
    if rows == 1 and out.stride(0) >= n:
        ldo = out.stride(0)
    return out, po, ldo


def _run(library: _Library, name: str, args, device: int, time):
    """time None: mmh_<name>(*args, stream).  time = (warmup, reps): mmh_time_<name>'s mean milliseconds per call."""
    if time is None:
        return library.check(getattr(library.lib(), "mmh_" + name)(*args, _stream(device)), "mmh_" + name)
    ms = C.c_float(0.0)
    library.check(getattr(library.lib(), "mmh_time_" + name)(*args, time[0], time[1], _stream(device), C.byref(ms)), "mmh_time_" + name)
    return ms.value


def _linear_s8o(what, x: QRows, qweight, bias, activation, so, inv, out=None, time=None):
    """mmh_q8o_linear (time = (warmup, reps): mmh_time_q8o_linear) on a QRows with the output scales `so` and their
    reciprocals `inv` (rows floats each): the QRows of the output, in `out` or in new rows of pitch out_features rounded up to 16."""
    _no_tiles4(what, qweight)   # (its packed image is not the (in_features, pitch) image this kernel reads)
    act = _activation_id(activation, what)
    rows, pxq, ldq, prx = _rows_args(what, x, qweight)
    n = qweight.out_features
    out, pyq, ldyq = _out_window(what, out, rows, n, True, qweight.device)
    pq, _, pr = qweight._ptrs
    args = (qweight.device, rows, n, qweight.in_features, pxq, ldq, prx, pq, qweight.pitch, pr, _bias_ptr(what, bias, qweight), act,
            so.data_ptr(), pyq, ldyq)
    ms = _run(_q8o, "q8o_linear", args, qweight.device, time) if time is not None or rows > 0 else None
    return ms if time is not None else QRows._of_window(out, inv[:rows], pyq, ldyq)


def _linear_args(what, x, qweight, bias, activation, out):
    """mmh_q8_linear's arguments between the object and the stream, and `out`."""
    import torch
    act = _activation_id(activation, what)
    _float_rows(what, x, qweight)
    rows, dev = x.shape[0], qweight.device
    if out is None:
        out = torch.empty((rows, qweight.out_features), dtype=torch.float32, device=x.device)
    px, ldx = tensor_args(x, rows, qweight.in_features, what + "(x)", torch.float32, dev)
    py, ldy = tensor_args(out, rows, qweight.out_features, what + "(out)", torch.float32, dev)
    return (rows, px, ldx, _bias_ptr(what, bias, qweight), act, py, ldy), out


def _no_tiles4(what, qweight) -> None:
    if isinstance(qweight, QWeight4):
        raise MMultError(ERR_UNSUPPORTED, what, "a QWeight4 has no tile path: 4-bit weights run through qlinear_decode, 1 - "
                         f"{Q4D_MAX_ROWS} rows per call")


def qlinear(x, qweight: QWeight, bias=None, activation=None, out=None, out_scale=None):
    """y = act(x @ w.t() + bias) in int8 (the headers' contracts).  x: (rows, in_features) fp32, quantised per row on the way
    in, or a QRows, read as it is (no quantiser pass; one QRows may feed any number of weights).  bias (out_features,) or
    None; activation None or "relu".  out_scale None: y is fp32, `out` (rows, out_features) fp32 of any row stride.
    out_scale a Python float or a (rows,) fp32 device tensor: y is quantised with that scale per row and returned as a QRows
    -- q in `out`, an int8 (rows, out_features) window of any pitch and base, or in new rows of pitch out_features rounded up to 16; inv_scale =
    fl(1 / out_scale) --, which the next qlinear reads in place."""
    _no_tiles4("qlinear", qweight)
    if out_scale is not None:
        if not isinstance(x, QRows):
            _float_rows("qlinear", x, qweight)
            x = quantize(x)
        so, inv = _scale_vectors("qlinear", out_scale, x.rows, qweight.device)
        return _linear_s8o("qlinear", x, qweight, bias, activation, so, inv, out)
    if isinstance(x, QRows):
        args, out = _linear_s8_args("qlinear", x, qweight, bias, activation, out)
        if args[0] > 0:
            _run(_q8, "q8_linear_s8", (qweight._handle, *args), qweight.device, None)
        return out
    args, out = _linear_args("qlinear", x, qweight, bias, activation, out)
    if args[0] > 0:
        _run(_q8, "q8_linear", (qweight._handle, *args), qweight.device, None)
    return out


def time_qlinear(x, qweight: QWeight, bias=None, activation=None, out=None, warmup: int = 1, reps: int = 20) -> float:
    """Mean milliseconds per qlinear call (one event pair around `reps` calls)."""
    _no_tiles4("time_qlinear", qweight)
    args, _ = _linear_args("time_qlinear", x, qweight, bias, activation, out)
    return _run(_q8, "q8_linear", (qweight._handle, *args), qweight.device, (warmup, reps))


def time_qlinear_s8o(x: QRows, qweight: QWeight, bias=None, activation=None, out=None, out_scale=1.0, warmup: int = 1, reps: int = 20) -> float:
    """Mean milliseconds per int8-output qlinear call on a QRows (one event pair around `reps` calls)."""
    _no_tiles4("time_qlinear_s8o", qweight)
    so, inv = _scale_vectors("time_qlinear_s8o", out_scale, x.rows, qweight.device)
    return _linear_s8o("time_qlinear_s8o", x, qweight, bias, activation, so, inv, out, time=(warmup, reps))


_cu_counts = {}


def _cu_count(device: int) -> int:
    """The device's compute units (what the decode plan fills), asked of torch once per device."""
    import torch
    if device not in _cu_counts:
        _cu_counts[device] = int(torch.cuda.get_device_properties(device).multi_processor_count)
    return _cu_counts[device]


def _linear_q8d(what, x: QRows, qweight, bias, activation, so, inv, out=None, splits=0, time=None):
    """mmh_q8d_linear (time = (warmup, reps): mmh_time_q8d_linear) on a QRows of at most 16 rows.  so None: the fp32 result in
    `out` or a new dense tensor; else the output scales `so` and their reciprocals `inv` (rows floats each) and the QRows of the
    output, in `out` or in new rows of pitch out_features rounded up to 16.  The partials go through the weight's workspace."""
    act = _activation_id(activation, what)
    rows, pxq, ldq, prx = _rows_args(what, x, qweight)
    four, grouped = isinstance(qweight, QWeight4), isinstance(qweight, QWeight4G)
    if rows > Q8D_MAX_ROWS:
        raise MMultError(ERR_UNSUPPORTED, what, _too_many_rows(qweight))
    n, k = qweight.out_features, qweight.in_features
    out8 = so is not None
    out, po, ldo = _out_window(what, out, rows, n, out8, qweight.device)
    if rows == 0 or n == 0:
        if time is not None:
            raise MMultError(ERR_INVALID_ARG, what, "nothing to time")
        return QRows._of_window(out, inv[:rows], po, ldo) if out8 else out
    pq, _, pr = qweight._ptrs
    work_bytes = 0
    if k > 0:
        extra = {"pitch_s": qweight.pitch_s, "gs_mod16": pr % 16} if grouped else {}
        work_bytes = qweight._decode_plan(rows, n, k, ldq, qweight.pitch, out8, ldo, 0, pq % 4, po % 16, splits, _cu_count(qweight.device),
                                          **extra)[1]
    work = qweight._decode_workspace(work_bytes) if k > 0 else None
    scales = (pr, qweight.pitch_s) if grouped else (pr,)   # one factor per group and channel, or one per channel
    args = (qweight.device, rows, n, k, pxq, ldq, prx, pq, qweight.pitch, *scales, _bias_ptr(what, bias, qweight), act,
            so.data_ptr() if out8 else None, None if out8 else po, 0 if out8 else ldo, po if out8 else None, ldo if out8 else 0,
            work.data_ptr() if work is not None else None, work.numel() if work is not None else 0, splits)
    if grouped:
        ms = _run(_q4g, "q4g_linear", args, qweight.device, time)
    else:
        ms = _run(_q4d, "q4d_linear", args, qweight.device, time) if four else _run(_q8d, "q8d_linear", args, qweight.device, time)
    if time is not None:
        return ms
    return QRows._of_window(out, inv[:rows], po, ldo) if out8 else out


def _too_many_rows(qweight) -> str:
    if isinstance(qweight, QWeight4):
        return f"at most {Q4D_MAX_ROWS} rows -- there are no 4-bit tiles for larger batches"
    return f"at most {Q8D_MAX_ROWS} rows -- larger batches are qlinear's"


def _decode_rows(what, x, qweight) -> QRows:
    """x as the QRows the decode kernels read: itself, or quantize(x) of an fp32 (rows <= 16, in_features) tensor."""
    if isinstance(x, QRows):
        return x
    _float_rows(what, x, qweight)
    if x.shape[0] > Q8D_MAX_ROWS:
        raise MMultError(ERR_UNSUPPORTED, what, _too_many_rows(qweight))
    return quantize(x)


def qlinear_decode(x, qweight: QWeight, bias=None, activation=None, out=None, out_scale=None, splits: int = 0):
    """qlinear for 1 - 16 rows (libmmult_hip_q8d.so; a QWeight4: libmmult_hip_q4d.so, the same arguments, the bits of the int8
    layer on the unpacked image): the same arguments, the same bits -- the weight is streamed once by
    strips x K ranges of workgroups (split-K; int32 partials add up exactly), a second kernel applies the epilogue.  x fp32 is
    quantised first with quantize(); a QRows is read in place.  More than 16 rows raise MMultError.  splits: 0 the plan's
    choice, > 0 that many K ranges.  The partials live in a workspace cached on `qweight`: it grows on demand, but not under
    graph capture -- QWeight.reserve_decode() sizes it first.
    A QWeight4G (libmmult_hip_q4g.so) has a bit contract of its own (include/mmult_hip_q4g.h): its partials are fp32 sums of
    group terms, added in group order inside a K range and in range order across ranges, so THE BITS DEPEND ON THE PARTITION
    (splits, k_len).  The partition is the plan's (qlinear_decode4g_plan: host arithmetic, no device needed); with splits=0 it
    depends on the row count and on the device's CU count, so force `splits` to get the same bits at every batch size and on
    every part."""
    x = _decode_rows("qlinear_decode", x, qweight)
    so = inv = None
    if out_scale is not None:
        so, inv = _scale_vectors("qlinear_decode", out_scale, x.rows, qweight.device)
    return _linear_q8d("qlinear_decode", x, qweight, bias, activation, so, inv, out, splits)


def time_qlinear_decode(x: QRows, qweight: QWeight, bias=None, activation=None, out=None, out_scale=None, splits: int = 0,
                        warmup: int = 1, reps: int = 20) -> float:
    """Mean milliseconds per qlinear_decode call on a QRows (one event pair around `reps` calls)."""
    so = inv = None
    if out_scale is not None:
        so, inv = _scale_vectors("time_qlinear_decode", out_scale, x.rows, qweight.device)
    return _linear_q8d("time_qlinear_decode", x, qweight, bias, activation, so, inv, out, splits, time=(warmup, reps))


def scale_of_amax(amax: float) -> float:
    """The quantiser's scale of a maximum, in float32: 127 / amax; 1 when amax is not above 0; clamped to FLT_MAX."""
    import numpy as np
    a = np.float32(amax)
    if not a > 0:
        return 1.0
    with np.errstate(all="ignore"):
        s = np.float32(127.0) / a
    return float(min(s, np.finfo(np.float32).max))


def _make_qmlp_class():
    import torch

    class QMLP(torch.nn.Module):
        """A stack of linear layers in int8, inference only: one row quantiser, then int8 -> int8 for every hidden layer (the
        GEMM's epilogue writes the next layer's rows: no fp32 activation ever reaches memory), then int8 -> fp32 for the last.
        The hidden activations are quantised with one static scale per layer (`out_scales`): calibrate(x) measures them, or
        set them by hand.  `activation` follows every hidden layer, `last_activation` the last.  A stack that holds a QWeight4
        needs decode=True and takes at most 16 rows per call, in forward and in calibrate: 4-bit weights have no tile path."""

        def __init__(self, qweights, biases=None, activation="relu", last_activation=None, decode=False):
            super().__init__()
            self.decode = bool(decode)   # batches of at most 16 rows go through qlinear_decode (the same bits)
            _activation_id(activation, "QMLP")
            _activation_id(last_activation, "QMLP")
            self.qweights = list(qweights)
            if not self.qweights:
                raise MMultError(ERR_INVALID_ARG, "QMLP", "need at least one QWeight")
            self._four = any(isinstance(q, QWeight4) for q in self.qweights)   # every call goes through qlinear_decode
            if self._four and not self.decode:
                raise MMultError(ERR_INVALID_ARG, "QMLP", "a QWeight4 in the stack needs decode=True (4-bit weights have no tile path)")
            biases = list(biases) if biases is not None else [None] * len(self.qweights)
            for a, b in zip(self.qweights, self.qweights[1:]):
                if a.out_features != b.in_features or a.device != b.device:
                    raise MMultError(ERR_INVALID_ARG, "QMLP", "each layer reads what the one before it writes, on one device")
            if len(biases) != len(self.qweights):
                raise MMultError(ERR_INVALID_ARG, "QMLP", "one bias (or None) per layer")
            for i, b in enumerate(biases):
                self.register_buffer(f"bias{i}", b)
            self.activation, self.last_activation = activation, last_activation
            self.in_features, self.out_features = self.qweights[0].in_features, self.qweights[-1].out_features
            self._out_scales = [] if len(self.qweights) == 1 else None
            self._vectors, self._vector_rows = [], 0   # per hidden layer (so, fl(1 / so)), constant vectors of _vector_rows rows

        @classmethod
        def from_float(cls, linears, activation="relu", last_activation=None, decode=False):
            """The int8 stack of torch.nn.Linear layers whose weights live on a GPU."""
            linears = list(linears)
            dev = linears[0].weight.device
            return cls([QWeight(l.weight.detach()) for l in linears],
                       [None if l.bias is None else l.bias.detach().to(torch.float32).to(dev).contiguous() for l in linears],
                       activation, last_activation, decode)

        def _bias(self, i):
            return getattr(self, f"bias{i}")

        @property
        def out_scales(self):
            """One output scale per hidden layer (Python floats, float32 values), or None before calibrate()."""
            return None if self._out_scales is None else list(self._out_scales)

        @out_scales.setter
        def out_scales(self, scales):
            import numpy as np
            scales = [float(np.float32(s)) for s in scales]
            if len(scales) != len(self.qweights) - 1 or not all(np.isfinite(s) and s > 0 for s in scales):
                raise MMultError(ERR_INVALID_ARG, "QMLP.out_scales", "one finite positive scale per hidden layer")
            self._out_scales, self._vectors, self._vector_rows = scales, [], 0

        def _rows(self, x):
            if x.requires_grad:
                raise MMultError(ERR_INVALID_ARG, "QMLP", "the int8 layers have no backward: x requires grad")
            rows = x.reshape(-1, self.in_features)
            if self._four and rows.shape[0] > Q4D_MAX_ROWS:   # before anything is launched
                raise MMultError(ERR_UNSUPPORTED, "QMLP", f"the stack holds 4-bit weights: at most {Q4D_MAX_ROWS} rows per call -- there "
                                 "are no 4-bit tiles for larger batches")
            if rows.shape[0] > 1 and rows.shape[1] > 1 and rows.stride(1) != 1:
                rows = rows.contiguous()
            return rows

        def _grow(self, rows):
            """The constant scale and reciprocal vectors hold `rows` rows (they allocate: not while capturing)."""
            if rows <= self._vector_rows:
                return
            dev = self.qweights[0].device
            if torch.cuda.is_current_stream_capturing():
                raise MMultError(ERR_UNSUPPORTED, "QMLP", "the scale vectors would have to grow while the stream is capturing -- "
                                 "run one uncaptured forward at the largest size first")
            self._vectors = [_scale_vectors("QMLP", s, rows, dev) for s in self._out_scales]
            self._vector_rows = rows

        def calibrate(self, x):
            """Run the layers with fp32 outputs on `x` and set each hidden layer's output scale to scale_of_amax of the
            largest finite |h| it produced.  Returns the scales.  At most 16 rows of a decode=True stack go through
            qlinear_decode (the same bits; the only route of a QWeight4)."""
            h = self._rows(x)
            layer = qlinear_decode if self.decode and h.shape[0] <= Q8D_MAX_ROWS else qlinear
            scales = []
            for i, qw in enumerate(self.qweights[:-1]):
                h = layer(h, qw, self._bias(i), self.activation)
                a = h.abs()
                amax = torch.where(torch.isfinite(a), a, torch.zeros_like(a)).max().item() if h.numel() else 0.0
                scales.append(scale_of_amax(amax))
            self.out_scales = scales
            self._grow(h.shape[0])
            return self.out_scales

        def forward(self, x):
            if self._out_scales is None:
                raise MMultError(ERR_INVALID_ARG, "QMLP", "no output scales: calibrate(x), or set out_scales, first")
            rows = self._rows(x)
            self._grow(rows.shape[0])
            h = quantize(rows)
            decode = self.decode and rows.shape[0] <= Q8D_MAX_ROWS
            for i, qw in enumerate(self.qweights[:-1]):
                so, inv = self._vectors[i]
                h = _linear_q8d("QMLP", h, qw, self._bias(i), self.activation, so, inv) if decode else \
                    _linear_s8o("QMLP", h, qw, self._bias(i), self.activation, so, inv)
            y = (qlinear_decode if decode else qlinear)(h, self.qweights[-1], self._bias(len(self.qweights) - 1), self.last_activation)
            return y.reshape(*x.shape[:-1], self.out_features)

        def extra_repr(self) -> str:
            dims = [self.in_features] + [q.out_features for q in self.qweights]
            return f"{' -> '.join(map(str, dims))}, activation={self.activation}, last_activation={self.last_activation}, out_scales={self._out_scales}"

    return QMLP


def _make_qlinear_class():
    import torch

    class QLinear(torch.nn.Module):
        """torch.nn.Linear (+ ReLU) in int8, inference only: the weight is a QWeight (set_weight / from_float), the bias an
        fp32 buffer.  forward flattens leading dimensions to rows; an input that requires grad raises."""

        def __init__(self, in_features: int, out_features: int, bias: bool = True, activation=None, decode: bool = False,
                     weight_bits: int = 8, group_size=None):
            super().__init__()
            self.decode = bool(decode)   # batches of at most 16 rows go through qlinear_decode (the same bits)
            if weight_bits not in (8, 4) or (weight_bits == 4 and not decode):
                raise MMultError(ERR_INVALID_ARG, "QLinear", "weight_bits is 8, or 4 with decode=True (4-bit weights have no tile path)")
            if group_size is not None and (weight_bits != 4 or group_size != Q4G_GROUP):
                raise MMultError(ERR_INVALID_ARG, "QLinear", f"group_size is None, or {Q4G_GROUP} with weight_bits=4 (a QWeight4G)")
            self.weight_bits = weight_bits   # 4: a QWeight4 -- every call goes through qlinear_decode, more than 16 rows are refused
            self.group_size = group_size     # 128: a QWeight4G, one scale per group of 128 input features
            _activation_id(activation, "QLinear")
            self.in_features, self.out_features, self.activation = in_features, out_features, activation
            self.qweight = None
            self.register_buffer("bias", torch.zeros(out_features) if bias else None)

        def set_weight(self, w, bias=None):
            """Prepare `w` (out_features, in_features) fp32 on a GPU; `bias` replaces the bias buffer's values."""
            if tuple(w.shape) != (self.out_features, self.in_features):
                raise MMultError(ERR_INVALID_ARG, "QLinear.set_weight", f"need a ({self.out_features},{self.in_features}) weight")
            self.qweight = (QWeight4G(w, self.group_size) if self.group_size else QWeight4(w)) if self.weight_bits == 4 else QWeight(w)
            if self.bias is not None:
                self.bias = (torch.zeros(self.out_features) if bias is None else bias.detach().to(torch.float32)).to(w.device).contiguous()
            return self

        @classmethod
        def from_float(cls, linear, activation=None, decode=False, weight_bits=8, group_size=None):
            """The int8 layer of a torch.nn.Linear whose weight lives on a GPU (weight_bits=4 with decode=True: 4-bit weights;
            group_size=128 with them: one scale per group of 128 input features)."""
            return cls(linear.in_features, linear.out_features, linear.bias is not None, activation, decode, weight_bits, group_size).set_weight(
                linear.weight.detach(), None if linear.bias is None else linear.bias.detach())

        def forward(self, x):
            if self.qweight is None:
                raise MMultError(ERR_INVALID_ARG, "QLinear", "no weight prepared: set_weight() or from_float() first")
            if x.requires_grad:
                raise MMultError(ERR_INVALID_ARG, "QLinear", "the int8 layer has no backward: x requires grad")
            rows = x.reshape(-1, self.in_features)
            if rows.shape[0] > 1 and rows.shape[1] > 1 and rows.stride(1) != 1:
                rows = rows.contiguous()
            layer = qlinear_decode if self.weight_bits == 4 or (self.decode and rows.shape[0] <= Q8D_MAX_ROWS) else qlinear
            y = layer(rows, self.qweight, self.bias, self.activation)
            return y.reshape(*x.shape[:-1], self.out_features)

        def extra_repr(self) -> str:
            return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, activation={self.activation}"

    return QLinear


def __getattr__(name):   # QLinear / QMLP are torch.nn.Modules: made when first asked for, so that importing this module does not import torch
    if name in ("QLinear", "QMLP"):
        cls = globals()[name] = (_make_qlinear_class if name == "QLinear" else _make_qmlp_class)()
        return cls
    raise AttributeError(name)


__all__ = ["QWeight", "QLinear", "QRows", "QMLP", "quantize_rows", "quantize", "qlinear", "time_qlinear", "time_qlinear_s8o", "qlinear_plan",
           "qlinear_s8o_plan", "scale_of_amax", "last_launch", "last_launch_q8o", "lib", "lib_q8o", "EXPORTS", "LIB_PATH", "HEADER",
           "Q8O_LIB_PATH", "Q8O_HEADER", "qlinear_decode", "time_qlinear_decode", "qlinear_decode_plan", "last_launch_q8d", "lib_q8d",
           "Q8D_LIB_PATH", "Q8D_HEADER", "Q8D_MAX_ROWS", "QWeight4", "weight4_layout", "qlinear_decode4_plan", "last_launch_q4d", "lib_q4d",
           "Q4D_LIB_PATH", "Q4D_HEADER", "Q4D_MAX_ROWS", "QWeight4G", "weight4g_layout", "qlinear_decode4g_plan", "last_launch_q4g", "lib_q4g",
           "Q4G_LIB_PATH", "Q4G_HEADER", "Q4G_GROUP"]
