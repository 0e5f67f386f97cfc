"""torch.autograd glue over MMult.linear / MMult.linear_backward: a linear layer (+ ReLU) that can be trained through.

    from how_to_optimize_gemm_amd import MMult, autograd
    mm = MMult(0, "auto")
    layer = autograd.Linear(mm, 1024, 4096, activation="relu").cuda()
    layer(x).sum().backward()

Forward is MMult.linear (one fused-epilogue launch), backward MMult.linear_backward (one gate + bias-gradient pass and the
GEMMs the inputs that require grad need).  MMult.linear itself stays outside autograd; nothing here computes in torch.
"""
from __future__ import annotations

import math

import torch

from .api import ERR_INVALID_ARG, MMultError


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mm, activation, x, w, bias):
        y = mm.linear(x, w, bias, activation)
        ctx.mm = mm
        ctx.has_bias = bias is not None
        # the ReLU gate reads the forward OUTPUT; without an activation the backward needs x and w only
        ctx.save_for_backward(x, w, *((y,) if activation == "relu" else ()))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable   # the backward's kernels are outside autograd: a double backward raises
    def backward(ctx, grad_out):
        x, w, *rest = ctx.saved_tensors
        y = rest[0] if rest else None
        # an expanded gradient (y.sum().backward(): every stride 0) or any other view the kernels cannot address
        if grad_out.dim() != 2 or (grad_out.shape[1] > 1 and grad_out.stride(1) != 1) or \
                (grad_out.shape[0] > 1 and grad_out.stride(0) < max(grad_out.shape[1], 1)):
            # (an empty tensor is contiguous to torch whatever its strides: .contiguous() would hand the expanded one back)
            grad_out = grad_out.contiguous() if grad_out.numel() else grad_out.new_empty(grad_out.shape)
        need = (ctx.needs_input_grad[2], ctx.needs_input_grad[3], ctx.has_bias and ctx.needs_input_grad[4])
        dx, dw, db = ctx.mm.linear_backward(grad_out, x, w, y, need=need)
        return None, None, dx, dw, db


def linear(mm, x, w, bias=None, activation=None):
    """y = act(x @ w.t() + bias) through `mm` (an MMult), differentiable in x, w and bias: x (rows, in), w (out, in), bias
    (out,) or None, activation None or "relu"."""
    if activation not in (None, "relu"):
        raise MMultError(ERR_INVALID_ARG, "autograd.linear", "activation is None or 'relu'")
    return _LinearFn.apply(mm, activation, x, w, bias)


class Linear(torch.nn.Module):
    """torch.nn.Linear (+ ReLU) on an MMult handle: weight (out_features, in_features), bias (out_features,), initialised as
    torch.nn.Linear does.  The handle is not moved or copied with the module: keep both on the same device."""

    def __init__(self, mm, in_features: int, out_features: int, bias: bool = True, activation=None):
        super().__init__()
        if activation not in (None, "relu"):
            raise MMultError(ERR_INVALID_ARG, "autograd.Linear", "activation is None or 'relu'")
        self.mm, self.in_features, self.out_features, self.activation = mm, in_features, out_features, activation
        self.weight = torch.nn.Parameter(torch.empty((out_features, in_features), dtype=torch.float32))
        self.bias = torch.nn.Parameter(torch.empty(out_features, dtype=torch.float32)) if bias else None
        torch.nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:
            bound = 1.0 / math.sqrt(in_features) if in_features > 0 else 0.0
            torch.nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x):
        return linear(self.mm, x, self.weight, self.bias, self.activation)

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, " \
               f"activation={self.activation}"
