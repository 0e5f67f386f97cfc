"""Bit comparison of fp32 results, on the host and on the device.

Where shared test code lives: plain modules beside the tests whose names do not start with `test_` -- this one, ex_ref.py
(the epilogue's reference arithmetic), gpu_operands.py (device operands, handles, fixtures), built_lib.py (the built library
read on the CPU), kernel_tables.py (tile vocabulary and shape generators several tables share), splitk_ref.py and
relu_grad_ref.py.  A test module never imports a helper from another test module: a new per-instantiation table keeps its
rows and row builder in its own test_gpu_*.py and takes everything else from here.

"Bit for bit" is same_bits: the uint32 patterns are equal wherever the expectation is not NaN (so -0.0 is not +0.0), and
NaN stands where the expectation has NaN (payloads are not compared)."""
import numpy as np


def same_bits(got, want) -> bool:
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    if not np.array_equal(nan_g, nan_w):
        return False
    return np.array_equal(np.where(nan_g, 0, got.view(np.uint32)), np.where(nan_w, 0, want.view(np.uint32)))


def first_difference(got, want) -> str:
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    bad = (np.isnan(got) != np.isnan(want)) | (~np.isnan(want) & (got.view(np.uint32) != want.view(np.uint32)))
    idx = np.argwhere(bad)
    if len(idx) == 0:
        return "no difference"
    i, j = idx[0]
    return f"{len(idx)} elements differ, first C[{i},{j}] = {got[i, j]!r} ({got.view(np.uint32)[i, j]:#010x}), " \
           f"oracle {want[i, j]!r} ({want.view(np.uint32)[i, j]:#010x})"


def same_bits_on_device(got, want):
    """same_bits on device tensors."""
    import torch
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and \
        torch.equal(got.view(torch.int32).masked_fill(nan, 0), want.view(torch.int32).masked_fill(nan, 0))


def bits_equal_on_device(got, want):
    import torch
    return torch.equal(got.view(torch.int32), want.view(torch.int32))
