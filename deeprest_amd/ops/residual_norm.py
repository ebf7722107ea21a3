"""Fused dropout + residual-add + LayerNorm — hand-written HIP kernel on GPU.

The residual glue of the attention encoder: ``x = x + dropout(branch)``
followed by ``layer_norm(x)`` is one pass that reads ``branch`` and the
residual stream and writes the new residual stream and the normed tensor
(csrc/residual_norm.hip).  The dropout mask is Philox4x32-10 keyed on the
element index, so it is regenerated (never stored) in backward and a CPU
oracle reproduces it bit for bit:

  element e = row * D + col      counter = (lo32(e>>2), hi32(e>>2),
                                            lo32(stream), hi32(stream))
  key = (lo32(key), hi32(key))   element e uses output word e & 3
  keep iff word >= min(floor(p * 2^32), 2^32 - 1)

``(key, stream)`` is a 2-element int64 tensor.  On GPU the kernel reads it
from device memory — it is never passed by value, so a captured hipGraph
that contains the draw sees fresh values on every replay.
"""

from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

from .native import require_native

_M0 = np.uint64(0xD2511F53)
_M1 = np.uint64(0xCD9E8D57)
_W0 = 0x9E3779B9
_W1 = 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _check_p(p: float) -> float:
    p = float(p)
    if not (0.0 <= p < 1.0):
        raise ValueError(f"dropout p must be in [0, 1), got {p}")
    return p


def _keep_threshold(p: float) -> int:
    return min(int(math.floor(float(p) * 4294967296.0)), 0xFFFFFFFF)


def philox4x32_10(counter: Sequence[np.ndarray], key: Tuple[int, int]):
    """Philox4x32-10 over arrays of 32-bit counter words held in uint64.

    ``counter`` is four arrays (or scalars) of values < 2^32, ``key`` two
    Python ints < 2^32; returns the four output word arrays (uint64, < 2^32).
    """
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in counter)
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0 = _M0 * c0
        p1 = _M1 * c2
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO,
                          (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO)
        k0 = (k0 + _W0) & 0xFFFFFFFF
        k1 = (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox_keep_mask(key: int, stream: int, numel: Union[int, Sequence[int]],
                     p: float) -> torch.Tensor:
    """The kernel's dropout keep mask, computed on CPU with numpy.

    ``numel`` is an element count or a shape; the bit of an element depends
    only on its flat index, so the mask of a shape is the mask of its element
    count reshaped.  Returns a CPU bool tensor (True = kept).
    """
    p = _check_p(p)
    shape = (int(numel),) if isinstance(numel, (int, np.integer)) else tuple(numel)
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    stream = int(stream) & 0xFFFFFFFFFFFFFFFF
    groups = np.arange((n + 3) // 4, dtype=np.uint64)
    zeros = np.zeros_like(groups)
    words = philox4x32_10(
        (groups & _LO, groups >> _S32,
         zeros + np.uint64(stream & 0xFFFFFFFF), zeros + np.uint64(stream >> 32)),
        (key & 0xFFFFFFFF, key >> 32))
    flat = np.stack(words, axis=1).reshape(-1)[:n]      # element e -> word e & 3
    keep = flat >= np.uint64(_keep_threshold(p))
    return torch.from_numpy(keep.reshape(shape))


def _draw_seed(device) -> torch.Tensor:
    # follows torch.manual_seed, device work only (no .item(), capturable)
    return torch.randint(0, 2 ** 62, (2,), dtype=torch.int64, device=device)


def _resolve_seed(seed: Optional[torch.Tensor], p: float, training: bool,
                  device) -> Optional[torch.Tensor]:
    """The (key, stream) tensor when a mask applies, else None (nothing drawn)."""
    if not training or p == 0.0:
        return None
    if seed is None:
        return _draw_seed(device)
    if seed.dtype != torch.int64 or seed.numel() != 2:
        raise ValueError("seed must be an int64 tensor of 2 elements (key, stream)")
    return seed


def reference_dropout_add_layer_norm(
        branch: torch.Tensor, residual: torch.Tensor,
        weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
        p: float = 0.0, training: bool = False, eps: float = 1e-5,
        seed: Optional[torch.Tensor] = None):
    """Plain torch composition with the kernel's mask: the CPU path of the op
    and the numerics oracle.  ``weight is None`` gives ``(r_out, None)``."""
    p = _check_p(p)
    dt = torch.result_type(branch, residual)
    seed = _resolve_seed(seed, p, training, branch.device)
    if seed is None:
        r_out = residual + branch
    else:
        key, stream = (int(s) for s in seed.tolist())
        keep = philox_keep_mask(key, stream, tuple(branch.shape), p)
        keep = keep.to(device=branch.device, dtype=torch.float32)
        r_out = (residual.float() + branch.float() * keep * (1.0 / (1.0 - p))).to(dt)
    if weight is None:
        return r_out, None
    normed = F.layer_norm(r_out, (r_out.shape[-1],), weight.to(r_out.dtype),
                          bias.to(r_out.dtype), eps)
    return r_out, normed


class _DropoutAddLayerNorm(torch.autograd.Function):
    """weight/bias None -> dropout_add (one output); seed None -> no mask.
    Neither ``branch`` nor a mask is saved: backward recomputes xhat from the
    saved r_out and regenerates the mask from the seed tensor."""

    @staticmethod
    def forward(ctx, branch, residual, weight, bias, seed, p, eps):
        ext = require_native("dropout_add_layer_norm")
        r_out, normed, mean, rstd = ext.dropout_add_ln_forward(
            branch, residual, weight, bias, seed, float(p), float(eps))
        ctx.has_norm = weight is not None
        ctx.p = float(p)
        if ctx.has_norm:
            ctx.save_for_backward(r_out, weight, mean, rstd, seed)
            return r_out, normed
        ctx.save_for_backward(r_out, seed)
        return r_out

    @staticmethod
    def backward(ctx, grad_r_out, grad_normed=None):
        ext = require_native("dropout_add_layer_norm")
        if ctx.has_norm:
            r_out, weight, mean, rstd, seed = ctx.saved_tensors
            d_res, d_branch, dw, db = ext.dropout_add_ln_backward(
                grad_normed.contiguous(), grad_r_out.contiguous(), r_out,
                weight, mean, rstd, seed, ctx.p)
            return d_branch, d_res, dw, db, None, None, None
        r_out, seed = ctx.saved_tensors
        d_res, d_branch, _, _ = ext.dropout_add_ln_backward(
            None, grad_r_out.contiguous(), r_out, None, None, None, seed, ctx.p)
        return d_branch, d_res, None, None, None, None, None


def _fused(branch, residual, weight, bias, p, training, eps, seed):
    p = _check_p(p)
    seed = _resolve_seed(seed, p, training, branch.device)
    dt = torch.result_type(branch, residual)
    if weight is not None:
        weight = weight.float().contiguous()
        bias = bias.float().contiguous()
    return _DropoutAddLayerNorm.apply(
        branch.to(dt).contiguous(), residual.to(dt).contiguous(), weight, bias,
        seed, p, eps)


def dropout_add_layer_norm(branch: torch.Tensor, residual: torch.Tensor,
                           weight: torch.Tensor, bias: torch.Tensor,
                           p: float = 0.0, training: bool = False,
                           eps: float = 1e-5,
                           seed: Optional[torch.Tensor] = None
                           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``r_out = residual + dropout(branch, p)``; ``normed = layer_norm(r_out)``.

    ``seed``: optional int64 ``(key, stream)`` tensor on the inputs' device;
    drawn from the torch generator when absent (training with p > 0 only).
    """
    if branch.is_cuda:
        return _fused(branch, residual, weight, bias, p, training, eps, seed)
    return reference_dropout_add_layer_norm(branch, residual, weight, bias, p,
                                            training, eps, seed)


def dropout_add(branch: torch.Tensor, residual: torch.Tensor, p: float = 0.0,
                training: bool = False,
                seed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``residual + dropout(branch, p)`` with the same in-kernel mask."""
    if branch.is_cuda:
        return _fused(branch, residual, None, None, p, training, 0.0, seed)
    return reference_dropout_add_layer_norm(branch, residual, None, None, p,
                                            training, 0.0, seed)[0]
