"""Multi-head attention over the endpoint x time window.

The traffic encoder attends over the time axis of the encoded endpoint
window (north star: "multi-head attention over the endpoint x time window on
MFMA with LDS-staged tiles").  The forward is ONE fused HIP kernel per
(batch, head): QK^T on MFMA with K staged in LDS (XOR-swizzled), online
softmax in registers, PV on MFMA — no S x S score tensor is materialized.
It saves the per-row logsumexp so the backward can recompute P cheaply.

The backward is ONE fused kernel per (batch-head, 64-key tile) in a
TRANSPOSED layout — keys as MFMA rows, queries as columns — so S^T, dP^T and
dS^T share one C-fragment layout and the softmax-grad math is lane-local
(per-column lse and D-row); dK/dV accumulate in registers with exclusive
stores, dQ via fp32 atomics.  It recomputes P from the saved logsumexp
instead of storing the S x S score tensor (replaced a rocBLAS recompute-GEMM
chain: 1 ms -> 0.23 ms per step at the bench config).

Replaces and upgrades the reference's per-metric feature-mask "attention"
(reference: resource-estimation/qrnn.py:21-23,34).
"""

from __future__ import annotations

import math
from typing import Optional

import torch

from .native import require_native


def reference_mha(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                  scale: Optional[float] = None,
                  kv_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q,k,v: (B, H, T, D). Plain composition (the numerics oracle).

    ``kv_lengths`` (B,) int: sample b is valid at t < clamp(kv_lengths[b], 1,
    T).  Padded keys are absent (-inf before the softmax), padded q/k/v
    values are replaced by zero through a select before any arithmetic (a NaN
    there cannot reach a valid row), and output rows at or past the length
    are exact zeros.  Broadcasting only: no host read of the lengths."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if kv_lengths is None:
        s = torch.matmul(q, k.transpose(-1, -2)) * scale
        p = torch.softmax(s.float(), dim=-1).to(q.dtype)
        return torch.matmul(p, v)
    T = q.shape[2]
    L = kv_lengths.to(q.device).clamp(1, T)
    valid = torch.arange(T, device=q.device)[None, :] < L[:, None]     # (B, T)
    row = valid[:, None, :, None]                                      # (B,1,T,1)
    zero = torch.zeros((), dtype=q.dtype, device=q.device)
    q, k, v = (torch.where(row, t, zero) for t in (q, k, v))
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    s = s.float().masked_fill(~valid[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1).to(q.dtype)
    return torch.where(row, torch.matmul(p, v), zero)


class _MHAFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale):
        ext = require_native("mha_forward")
        o, lse = ext.mha_forward(q, k, v, float(scale))
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale = float(scale)
        return o

    @staticmethod
    def backward(ctx, grad_o):
        ext = require_native("mha_backward")
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = ext.mha_backward(q, k, v, o, grad_o.contiguous(), lse,
                                      ctx.scale)
        return dq.to(q.dtype), dk, dv, None


def mha_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                scale: Optional[float] = None,
                kv_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused attention forward; q,k,v: (B, H, T, D) contiguous.

    ``kv_lengths`` (B,) int32 on the inputs' device: per-sample valid
    lengths (see ``reference_mha``).  Inference only — the kernel is called
    outside the autograd node and the call raises when grad mode is on and
    an input requires grad.  The lengths are read on the device."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if kv_lengths is not None:
        if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
            raise RuntimeError(
                "mha_forward with kv_lengths is inference-only (no autograd)")
        if q.is_cuda:
            ext = require_native("mha_forward")
            o, _ = ext.mha_forward(q.contiguous(), k.contiguous(),
                                   v.contiguous(), float(scale), kv_lengths)
            return o
        return reference_mha(q, k, v, scale, kv_lengths)
    if q.is_cuda:
        return _MHAFunction.apply(q.contiguous(), k.contiguous(), v.contiguous(), scale)
    return reference_mha(q, k, v, scale)
