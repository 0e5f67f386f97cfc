"""MI355X-native SGEMM backend behind the reference's MY_MMult entry point.

Layout (only what the hot path needs):
  csrc/      hand-written gfx950 HIP kernels + the C-ABI shim (libmmult_hip.so)
  csrc_q8/   the int8 linear layer's kernels and C ABI (libmmult_hip_q8.so, include/mmult_hip_q8.h)
  csrc_q8o/  the int8-to-int8 layer's kernels and C ABI (libmmult_hip_q8o.so, include/mmult_hip_q8o.h)
  harness/   C++ host side: MY_MMult forwarder and the test_MMult sweep driver
  abi_header.py  include/mmult_hip.h parsed: every MMH_* constant, every prototype as ctypes types
  api.py     the ctypes binding, made from abi_header -- no hand-kept mirror -- (+ torch device-pointer glue)
  autograd.py torch.autograd glue: a linear layer (+ ReLU) that trains through MMult.linear / linear_backward
  q8.py      the int8 linear layer on torch tensors: QWeight, quantize_rows, qlinear, QLinear, QRows, QMLP (bindings read from their headers)
  shard.py   one-process-per-GPU row-panel shard over torch.distributed (RCCL)
  build.py   hipcc recipe
"""
from .api import *  # noqa: F401,F403
