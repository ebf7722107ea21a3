"""LayerNorm (fwd/bwd) — hand-written HIP kernel on GPU.

The kernels are the residual-norm ones (csrc/residual_norm.hip) with the add
compiled out: ``layer_norm(x)`` is ``dropout_add_layer_norm`` with no branch,
no ``r_out`` copy and no gradient arriving through ``r_out``.  Memory-bound:
one wave per row, vectorized IO, two-pass statistics over wave shuffles and
a fused affine; docs/KERNELS.md has the tiers.  Backward needs D <= 8192.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from .native import require_native


def reference_layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                         eps: float = 1e-5) -> torch.Tensor:
    return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        ext = require_native("layer_norm")
        _, y, mean, rstd = ext.dropout_add_ln_forward(
            None, x, weight, bias, None, 0.0, float(eps))
        ctx.save_for_backward(x, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        ext = require_native("layer_norm")
        x, weight, mean, rstd = ctx.saved_tensors
        dx, _, dw, db = ext.dropout_add_ln_backward(
            grad_y.contiguous(), None, x, weight, mean, rstd, None, 0.0)
        return dx, dw, db, None


def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
               eps: float = 1e-5) -> torch.Tensor:
    if x.is_cuda:
        return _LayerNorm.apply(
            x.contiguous(), weight.float().contiguous(), bias.float().contiguous(), eps
        )
    return reference_layer_norm(x, weight, bias, eps)
