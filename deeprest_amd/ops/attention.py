"""Multi-head attention over the endpoint x time window.

The traffic encoder attends over the time axis of the encoded endpoint
window (north star: "multi-head attention over the endpoint x time window on
MFMA with LDS-staged tiles").  Two entry points share one set of kernels
(``csrc/attention.hip``), which address their operands by (batch, head,
time) element strides:

``mha_packed(qkv, n_heads)`` is what the model calls.  It takes the qkv GEMM
output ``(B, T, 3*H*Dh)`` as it is and returns ``(B, T, H*Dh)``, the layout
the output projection reads: no copy of q, k, v or o, and one autograd node
whose backward writes a single ``(B, T, 3, H, Dh)`` dqkv.

``mha_forward(q, k, v)`` takes ``(B, H, T, D)`` contiguous tensors, and is
the only path with per-sample ``kv_lengths`` (inference).

Kernels.  With T <= 64 and Dh in {16, 32, 64} one wave holds a whole (batch,
head): every global access is a 16-byte piece of a (t, head) row, the softmax
is taken once over all keys, the probability accumulators are the next MFMA's
operand, transposed operands come from ``ds_read_b64_tr_b16`` on row-major LDS
images, and there is no block barrier.  The backward recomputes P from the
saved per-row logsumexp and writes dq, dk, dv itself in the IO dtype: no
atomics, so the result is deterministic.  Longer windows (and other head
sizes) run the flash-style bodies: one workgroup per 64-row query tile with an
online softmax forward, one per (head, 64-key tile) backward in a transposed
layout whose dQ contributions go out as fp32 atomics into a zeroed buffer.
No S x S score tensor is ever materialized.

Replaces and upgrades the reference's per-metric feature-mask "attention"
(reference: resource-estimation/qrnn.py:21-23,34).
"""

from __future__ import annotations

import math
from typing import Optional

import torch

from .native import require_native

# "auto": mha_packed runs the strided kernels on the packed tensor (GPU).
# "off": it runs the composition of views, mha_forward and the transposing
# reshape, as the CPU path always does.  For tests and tools.
PACKED_MODE = "auto"


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


def _bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


def reference_mha_step(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                       dout: Optional[torch.Tensor],
                       scale: Optional[float] = None,
                       kv_lengths: Optional[torch.Tensor] = None, *,
                       emulate: Optional[str] = None):
    """Attention forward and backward written out, no autograd.

    q, k, v, dout: ``(B, H, T, D)``.  Returns ``(o, lse, dq, dk, dv)``.

    ``emulate=None`` is the reference, in the dtype of the inputs (the tests
    pass float64)::

        S = q k^T * scale;  lse = logsumexp(S);  P = exp(S - lse);  o = P v
        Drow = rowsum(dout * o);  dS = P * (dout v^T - Drow) * scale
        dq = dS k;  dk = dS^T q;  dv = P^T dout

    With ``kv_lengths`` (B,) the semantics are those of :func:`reference_mha`:
    lengths clamped to [1, T], padded keys absent, padded q/k/v replaced by
    zero through a select, rows of ``o`` and ``lse`` at or past the length
    exactly zero.  That mode is forward only: ``dout`` must be None and the
    three gradients come back None.

    ``emulate="bf16"`` or ``"f32"`` (the IO dtype of the kernels) is an
    emulation of the arithmetic of ``csrc/attention.hip``: float32 throughout,
    with a bf16 round trip where the four kernels round.  Its distance from the
    float64 reference is the error the number formats commit on these inputs.
    The roundings, each with the line of the flash-style bodies it mirrors (the
    whole-head tile bodies round at the same places):

    - q, k, v, dout as MFMA operands: ``f2bf(... ldf(qb ...))`` of the q
      fragments, of the K / V^T staging (forward), of ``tk`` / ``tv`` and the
      ``q_lds`` / ``do_lds`` staging (backward); tile bodies ``ld8`` /
      ``pack8``.  For bf16 IO this changes nothing;
    - ``S * scale`` in float32 after the product (``s_acc[nt][i] * scale``);
    - the row sum ``l`` over the unrounded exponentials
      (``l_run[i] += group16_sum(p[0][i] + p[1][i])``), P rounded before
      ``P v`` (``f2bf(p[nt][i])`` into ``p_lds``; tile: ``acc_pair_frag``);
    - ``o`` divided by ``l`` after the product (``o_acc[nt][i] * inv_l``);
      ``lse = m + log(l)`` in float32;
    - ``Drow`` in float32 from the IO-dtype values of dout and of the stored o
      (``s += ldf(dob ...) * ldf(ob ...)``): dout is not operand-rounded here;
    - the backward's ``P = exp(S * scale - lse)`` with the stored float32 lse
      (``__expf(st[nt][i] * scale - l)``), rounded before ``P^T dout``
      (``f2bf(p)`` into ``my_p``);
    - ``dS = P * (dP - Drow) * scale`` from the unrounded P, rounded after the
      multiplication by ``scale`` (``f2bf(st[nt][i])``) before its three
      products;
    - bf16 IO: o, dq, dk, dv rounded to bf16 on store (``stf``; the flash dq
      is summed in float32 and cast once); f32 IO: nothing more.

    Not modelled: the order of the float32 sums inside an MFMA and across the
    flash-style key steps and dq atomics, the running maximum against which the
    flash forward rounds P (the emulation rounds against the final one: another
    sample of the same relative rounding), ``__expf`` / ``__logf``.
    """
    if emulate not in (None, "bf16", "f32"):
        raise ValueError(f"emulate must be None, 'bf16' or 'f32', got {emulate!r}")
    if kv_lengths is not None and dout is not None:
        raise ValueError("reference_mha_step with kv_lengths is forward only")
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    same = lambda x: x                                           # noqa: E731
    if emulate is None:
        op = io = same
    else:
        op = _bf16_round
        io = _bf16_round if emulate == "bf16" else same
        q, k, v = (io(t.float()) for t in (q, k, v))
        dout = None if dout is None else io(dout.float())
    T = q.shape[2]
    row = None
    if kv_lengths is not None:
        L = kv_lengths.to(q.device).clamp(1, T)
        valid = torch.arange(T, device=q.device)[None, :] < L[:, None]  # (B, T)
        row = valid[:, None, :, None]
        zero = torch.zeros((), dtype=q.dtype, device=q.device)
        q, k, v = (torch.where(row, t, zero) for t in (q, k, v))
    qo, ko, vo = op(q), op(k), op(v)

    s = torch.matmul(qo, ko.transpose(-1, -2)) * scale
    if row is not None:
        s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    if emulate is None:
        lse = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - lse[..., None])
        o = torch.matmul(p, vo)
    else:
        m = s.max(dim=-1).values
        e = torch.exp(s - m[..., None])
        l = e.sum(dim=-1)
        o = io(torch.matmul(op(e), vo) / l[..., None])
        lse = m + torch.log(l)
    if row is not None:
        o = torch.where(row, o, zero)
        lse = torch.where(row[..., 0], lse, zero)
        return o, lse, None, None, None
    if dout is None:
        return o, lse, None, None, None

    douto = op(dout)
    drow = (dout * o).sum(dim=-1, keepdim=True)
    if emulate is not None:
        p = torch.exp(s - lse[..., None])
    dp = torch.matmul(douto, vo.transpose(-1, -2))
    ds = op(p * (dp - drow) * scale)
    dq = io(torch.matmul(ds, ko))
    dk = io(torch.matmul(ds.transpose(-1, -2), qo))
    dv = io(torch.matmul(op(p).transpose(-1, -2), douto))
    return o, lse, dq, dk, dv


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


class _MHAPackedFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, n_heads, scale):
        ext = require_native("mha_packed_forward")
        o, lse = ext.mha_packed_forward(qkv, int(n_heads), float(scale))
        ctx.save_for_backward(qkv, o, lse)
        ctx.n_heads = int(n_heads)
        ctx.scale = float(scale)
        return o

    @staticmethod
    def backward(ctx, grad_o):
        ext = require_native("mha_packed_backward")
        qkv, o, lse = ctx.saved_tensors
        grad_o = grad_o.contiguous()
        if grad_o.data_ptr() % 16:          # a view at an odd offset
            grad_o = grad_o.clone()
        dqkv = ext.mha_packed_backward(qkv, ctx.n_heads, o, grad_o, lse, ctx.scale)
        return dqkv.view(qkv.shape), None, None


def _mha_unpacked(qkv: torch.Tensor, n_heads: int,
                  scale: Optional[float]) -> torch.Tensor:
    B, T = qkv.shape[0], qkv.shape[1]
    qkv5 = qkv.view(B, T, 3, n_heads, -1)
    q, k, v = (qkv5[:, :, i].transpose(1, 2) for i in range(3))    # (B,h,T,dh)
    attn = mha_forward(q, k, v, scale)
    return attn.transpose(1, 2).reshape(B, T, -1)


def mha_packed(qkv: torch.Tensor, n_heads: int,
               scale: Optional[float] = None) -> torch.Tensor:
    """Attention on the packed qkv projection.

    ``qkv``: ``(B, T, 3*H*Dh)`` or ``(B, T, 3, H, Dh)`` contiguous, bf16 or
    f32, Dh a multiple of 8 in 8..64 on the GPU; returns ``(B, T, H*Dh)``
    contiguous.  On the GPU the kernels read q, k, v in place and write the
    output and, in the backward, one dqkv tensor directly; a bad operand
    raises before any launch.  On the CPU, and with ``PACKED_MODE = "off"``,
    it is the composition of the three views, ``mha_forward`` and the
    transposing reshape."""
    if PACKED_MODE not in ("auto", "off"):
        raise ValueError(f"PACKED_MODE must be 'auto' or 'off', got {PACKED_MODE!r}")
    if qkv.is_cuda and PACKED_MODE == "auto":
        if qkv.dim() not in (3, 5):
            raise RuntimeError("qkv must be (B, T, 3*H*Dh) or (B, T, 3, H, Dh)")
        if scale is None:
            last = qkv.shape[-1] if qkv.dim() == 5 else qkv.shape[-1] // (3 * n_heads)
            scale = 1.0 / math.sqrt(max(last, 1))
        return _MHAPackedFunction.apply(qkv, n_heads, scale)
    return _mha_unpacked(qkv, n_heads, scale)
