"""Fused GRU sequence op.

The per-resource GRU decoders dominate the training step (SURVEY.md section 7:
"the fused GRU cell first — it dominates runtime").  Design:

- the input-side projection (x @ W_ih^T + b_ih) is a plain large GEMM done
  once for the whole sequence by rocBLAS/hipBLASLt *outside* this op;
- this op consumes those precomputed input gates ``x_gates (B, T, 3H)``,
  broadcasts them over C per-component decoders through a FiLM condition
  (gamma/beta per component), and runs the *recurrent* part — per time step
  a (B*C, H) x (H, 3H) MFMA GEMM fused with the sigmoid/tanh gate math —
  entirely inside ONE kernel launch for the whole sequence.  Rows evolve
  independently, so there is no cross-workgroup dependency: each workgroup
  keeps its row tile's hidden state in registers, stages W_hh in LDS once,
  and loops over T.

Gate layout follows PyTorch nn.GRU (r, z, n) so the CPU oracle can be
checked against torch.nn.GRUCell:

    r = sigmoid(xg_r + h W_hr + b_hr)
    z = sigmoid(xg_z + h W_hz + b_hz)
    n = tanh(xg_n + r * (h W_hn + b_hn))
    h' = (1 - z) * n + z * h

Replaces the cuDNN GRU call of the reference (reference:
resource-estimation/qrnn.py:24,41) — and allocates hidden state on-device,
avoiding the reference's CPU-hidden-state bug (qrnn.py:39-40).
"""

from __future__ import annotations

from typing import Optional

import torch

from .native import require_native

# constant pi-permutation index tensors, cached per device (rebuilding them
# each backward call costs ~6 tiny kernel launches per direction per step)
_IDX_CACHE: dict = {}


def _pi_indices(device):
    key = str(device)
    got = _IDX_CACHE.get(key)
    if got is None:
        H = 128
        m = torch.arange(3 * H, device=device)
        g = m // H
        q = m % H
        col = (q % 8) * 16 + (q // 8)
        natj = torch.where(m < 2 * H, g * H + col, 2 * H + col)
        idx = torch.arange(4 * H, device=device)
        gg = idx // H
        qq = idx % H
        nat4 = gg * H + (qq % 8) * 16 + (qq // 8)  # dpre-row unpermute, 4H
        got = (natj, nat4)
        _IDX_CACHE[key] = got
    return got


def reference_gru_sequence(
    x_gates: torch.Tensor,       # (B, T, 3H) precomputed input gates
    w_hh: torch.Tensor,          # (3H, H) recurrent weight (PyTorch layout)
    b_hh: torch.Tensor,          # (3H,)
    h0: torch.Tensor,            # (B, C, H)
    gamma: Optional[torch.Tensor] = None,  # (C, 3H) FiLM scale
    beta: Optional[torch.Tensor] = None,   # (C, 3H) FiLM shift
    reverse: bool = False,
    lengths: Optional[torch.Tensor] = None,   # (B,) int per-sample lengths
    return_state: bool = False,
):
    """Differentiable PyTorch composition; returns h_all (B, T, C, H).

    ``lengths``: sample b is valid at t < clamp(lengths[b], 1, T).  At a
    padded step the sample HOLDS its state through ``torch.where`` (whatever
    the padded x_gates hold, NaN included, is computed and discarded) and
    its h_all entry is zero; so the reverse direction starts from h0 at each
    sample's own last step.  ``return_state=True`` returns ``(h_all, h)``
    with ``h`` the final held state (B, C, H)."""
    B, T, G = x_gates.shape
    _, C, H = h0.shape
    assert G == 3 * H, f"x_gates last dim {G} != 3*H ({3 * H})"
    h = h0
    outs = []
    if lengths is not None:
        lengths = lengths.to(x_gates.device).clamp(1, T)
    steps = range(T - 1, -1, -1) if reverse else range(T)
    w_hh_t = w_hh.t()  # (H, 3H)
    for t in steps:
        g = x_gates[:, t, None, :]                      # (B, 1, 3H)
        if gamma is not None:
            g = g * gamma[None] + (beta[None] if beta is not None else 0.0)
        else:
            g = g.expand(B, C, G)
        hh = h @ w_hh_t + b_hh                          # (B, C, 3H)
        r = torch.sigmoid(g[..., :H] + hh[..., :H])
        z = torch.sigmoid(g[..., H : 2 * H] + hh[..., H : 2 * H])
        n = torch.tanh(g[..., 2 * H :] + r * hh[..., 2 * H :])
        h_new = (1.0 - z) * n + z * h
        if lengths is None:
            h = h_new
            outs.append(h)
        else:
            active = (lengths > t)[:, None, None]       # (B, 1, 1), on device
            h = torch.where(active, h_new, h)
            outs.append(torch.where(active, h_new, torch.zeros_like(h_new)))
    if reverse:
        outs.reverse()
    h_all = torch.stack(outs, dim=1)                    # (B, T, C, H)
    return (h_all, h) if return_state else h_all


class _FusedGRUSequence(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_gates, w_hh, b_hh, h0, gamma, beta, reverse):
        ext = require_native("fused_gru_sequence")
        # NOTE: grad mode is disabled inside Function.forward, so
        # torch.is_grad_enabled() is useless here — ctx.needs_input_grad is
        # the correct signal for whether backward will run.
        need_grad = any(ctx.needs_input_grad)
        h_all, saves = ext.gru_seq_forward(
            x_gates, w_hh, b_hh, h0, gamma, beta, bool(reverse), bool(need_grad)
        )
        ctx.save_for_backward(x_gates, w_hh, b_hh, h0, gamma, beta, h_all, saves)
        ctx.reverse = bool(reverse)
        return h_all

    @staticmethod
    def backward(ctx, grad_h_all):
        ext = require_native("fused_gru_sequence")
        x_gates, w_hh, b_hh, h0, gamma, beta, h_all, saves = ctx.saved_tensors
        reverse = ctx.reverse
        w_img, w_fwd = _bwd_weight_images(w_hh)
        # sequential chain (custom kernel): dpre = [dr_pre|dz_pre|d_hh_n|dn_pre]
        dpre, dh0 = ext.gru_seq_backward_kernel(
            grad_h_all.contiguous(), w_img, w_fwd, x_gates, gamma, beta, b_hh,
            h0, h_all, saves, reverse
        )
        return _bwd_reductions(ext, dpre, dh0, x_gates, w_hh, h0, gamma, h_all,
                               reverse) + (None,)


def _bwd_weight_images(w_hh):
    """bf16 weight images the backward kernel reads: the pi-permuted W image
    (H, 3H) for the dh GEMM — row k holds W[natJ(m), k] over the MFMA K axis
    m (dr | dz | d_hhn regions) — and the natural (3H, H) image for the hh_n
    recompute GEMM.  Cast once, then gather/transpose in bf16 (fewer/smaller
    copies)."""
    natj, _ = _pi_indices(w_hh.device)
    w_fwd = w_hh.to(torch.bfloat16).contiguous()
    w_img = w_fwd[natj, :].t().contiguous()
    return w_img, w_fwd


# Which reduce kernels _bwd_reductions asks for: "auto" (the single pass
# wherever it applies), "split" or "fused".  Tests and tools/bench_gru_reduce.py
# set it to pin one path.
REDUCE_MODE = "auto"


def reference_bwd_reduce(dpre, gamma, xg):
    """What ext.gru_bwd_reduce computes, in plain torch and in the inputs'
    dtype (pass float64 for a reference): dpre (B, T, C, 4H) holds the
    pi-packed slices dr|dz|d_hhn|dn.  Returns, in the binding's layout,
    dxg (B, T, 3H), dgamma (C, 3H) and dbeta4 (C, 4H): columns in natural
    order, dbeta4's slices in dpre's order."""
    B, T, C, G4 = dpre.shape
    H = G4 // 4
    _, nat4 = _pi_indices(dpre.device)
    nat = torch.empty_like(dpre)
    nat.index_copy_(3, nat4, dpre)                      # unpermute each slice
    dx = torch.cat([nat[..., : 2 * H], nat[..., 3 * H:]], dim=-1)  # r|z|n
    dxg = (dx * gamma).sum(dim=2)
    dgamma = (dx * xg[:, :, None, :]).sum(dim=(0, 1))
    dbeta4 = nat.sum(dim=(0, 1))
    return dxg, dgamma, dbeta4


def _bwd_reductions(ext, dpre, dh0, x_gates, w_hh, h0, gamma, h_all, reverse):
    """Everything after the sequential chain, shared by the plain and the
    head-fused backward: returns (dxg, dw_hh, db_hh, dh0, dgamma, dbeta)."""
    B, T, C, G4 = dpre.shape
    H = G4 // 4

    # dpre rows use the kernel's pi packing: position g*128 + cc*8 + nt
    # holds natural column g*128 + nt*16 + cc — unpermute dW rows after
    # the GEMM (tiny index_copy on a (K, H) matrix).
    _, nat4 = _pi_indices(w_hh.device)

    # dW_hh = sum over (b,t,c) of [dr|dz|d_hhn]^T h_prev: dpre's first three
    # slices, so ONE batched strided GEMM (rocBLAS picks per-B batching =>
    # proper chip occupancy; no cats: the t=0/t=T-1 boundary term against h0
    # is a separate small bmm; at T = 1 the main part is empty and adds zero)
    if reverse:
        dp_main = dpre[:, :-1, :, : 3 * H]              # h_prev = h_all[t+1]
        h_main = h_all[:, 1:]
        dp_bound = dpre[:, -1, :, : 3 * H]              # h_prev = h0
    else:
        dp_main = dpre[:, 1:, :, : 3 * H]               # h_prev = h_all[t-1]
        h_main = h_all[:, :-1]
        dp_bound = dpre[:, 0, :, : 3 * H]
    a = dp_main.reshape(B, (T - 1) * C, 3 * H).transpose(1, 2)
    part = torch.bmm(a, h_main.reshape(B, (T - 1) * C, H))
    ab = dp_bound.reshape(B, C, 3 * H).transpose(1, 2)
    part = part + torch.bmm(ab, h0)
    dw_pi = part.sum(0, dtype=torch.float32)            # (3H, H), pi rows
    dw_hh = torch.empty_like(dw_pi)
    dw_hh.index_copy_(0, nat4[: 3 * H], dw_pi)          # natural rows r|z|n

    # reductions over dpre (custom kernels): dxg, dgamma, dbeta4.  dbeta4
    # follows dpre's slice order r|z|hh_n|n: the first three slices summed
    # over C are db_hh, slices r, z, n are dbeta.
    dxg, dgamma, dbeta4 = ext.gru_bwd_reduce(dpre, gamma, x_gates, REDUCE_MODE)
    db_hh = dbeta4[:, : 3 * H].sum(dim=0)               # (3H,) f32, tiny
    dbeta = torch.cat([dbeta4[:, : 2 * H], dbeta4[:, 3 * H:]], dim=1)
    return (
        dxg,
        dw_hh.to(w_hh.dtype),
        db_hh,
        dh0.to(h0.dtype),
        dgamma.to(gamma.dtype),
        dbeta.to(gamma.dtype),
    )


HEAD_FUSE_MAX_OUT = 32    # one K=32 MFMA covers the heads' output width


def _head_image_fwd(w_head):
    """(32, H) bf16 B-operand image of the forward kernels' head phase:
    w_head (O, H) rounded to bf16 and zero-padded along the output axis."""
    wh_fwd = torch.zeros(32, w_head.shape[1], device=w_head.device,
                         dtype=torch.bfloat16)
    wh_fwd[:w_head.shape[0]] = w_head
    return wh_fwd


class _FusedGRUHeads(torch.autograd.Function):
    """GRU sequence + quantile-head projection as one autograd node, so the
    backward never materializes the (B, T, C, H) head input gradient: the
    kernel rebuilds grad_part @ w_head per step on the matrix unit.  Where
    the saving forward kernel has a head phase (the binding knows), the
    forward projection runs per step inside it too."""

    @staticmethod
    def forward(ctx, x_gates, w_hh, b_hh, h0, gamma, beta, w_head, reverse):
        ext = require_native("fused_gru_heads")
        need_grad = any(ctx.needs_input_grad)
        args = (x_gates, w_hh, b_hh, h0, gamma, beta, bool(reverse), bool(need_grad))
        w = w_head.to(x_gates.dtype)
        B, C, H = h0.shape
        T = x_gates.shape[1]
        if ext.gru_fwd_fuses_heads(B, C, bool(need_grad)):
            # the kernel projects each step's h onto the heads itself (w_head
            # rounded to bf16, as in fused_gru_decode): h_all is not read back
            h_all, saves, part = ext.gru_seq_forward(
                *args, False, _head_image_fwd(w), w.shape[0])
        else:
            h_all, saves = ext.gru_seq_forward(*args)
            # same GEMM as ops/linear_bigk.py's forward (3-D, leading-dim batch)
            part = torch.matmul(h_all.reshape(B, T * C, H), w.t())
        ctx.save_for_backward(x_gates, w_hh, b_hh, h0, gamma, beta, h_all, saves, w)
        ctx.reverse = bool(reverse)
        ctx.w_head_dtype = w_head.dtype
        return part.reshape(B, T, C, w.shape[0])

    @staticmethod
    def backward(ctx, grad_part):
        ext = require_native("fused_gru_heads")
        (x_gates, w_hh, b_hh, h0, gamma, beta, h_all, saves,
         w) = ctx.saved_tensors
        reverse = ctx.reverse
        B, T, C, H = h_all.shape
        O = w.shape[0]
        g = grad_part.contiguous().to(h_all.dtype)
        w_img, w_fwd = _bwd_weight_images(w_hh)
        # (H, 32) bf16 B-operand image: w_head^T zero-padded along K
        wh_img = torch.zeros(H, 32, device=w.device, dtype=torch.bfloat16)
        wh_img[:, :O] = w.t()
        dpre, dh0 = ext.gru_seq_backward_heads_kernel(
            g, wh_img, w_img, w_fwd, x_gates, gamma, beta, b_hh, h0, h_all,
            saves, reverse
        )
        # dW_head as in ops/linear_bigk.py: leading-dim-batched GEMMs, fp32 sum
        dw_head = torch.bmm(g.reshape(B, T * C, O).transpose(1, 2),
                            h_all.reshape(B, T * C, H)).sum(0, dtype=torch.float32)
        return _bwd_reductions(ext, dpre, dh0, x_gates, w_hh, h0, gamma, h_all,
                               reverse) + (dw_head.to(ctx.w_head_dtype), None)


_WARNED_SHAPES = set()


def gru_kernel_supports(H: int, C: int) -> bool:
    """Shapes the fused CDNA4 kernel is built for: its LDS staging, MFMA
    tiling and pi-permutation are specialized to hidden size 128, and the
    64-row tile layout needs >= 3 components per batch row group."""
    return H == 128 and C >= 3


def _fuses_heads(x_gates, h0, w_head) -> bool:
    """The native kernel applies and the heads fit its one K=32 MFMA step
    (backward) / two 16-wide output tiles (decode)."""
    return (x_gates.is_cuda and gru_kernel_supports(h0.shape[2], h0.shape[1])
            and w_head.shape[0] <= HEAD_FUSE_MAX_OUT)


def _kernel_operands(x_gates, w_hh, b_hh, h0, gamma, beta):
    """The six operands as the kernel entries take them: contiguous, in
    x_gates' dtype, b_hh in fp32.  Called outside the autograd Functions so
    the casts are tracked back to the fp32 master parameters."""
    dt = x_gates.dtype
    return (
        x_gates.contiguous(),
        w_hh.to(dt).contiguous(),
        b_hh.float().contiguous(),
        h0.to(dt).contiguous(),
        gamma.to(dt).contiguous(),
        beta.to(dt).contiguous(),
    )


def fused_gru_sequence(
    x_gates: torch.Tensor,
    w_hh: torch.Tensor,
    b_hh: torch.Tensor,
    h0: torch.Tensor,
    gamma: Optional[torch.Tensor] = None,
    beta: Optional[torch.Tensor] = None,
    reverse: bool = False,
    fp8: bool = False,
) -> torch.Tensor:
    if x_gates.is_cuda and not gru_kernel_supports(h0.shape[2], h0.shape[1]):
        # Defined degradation path (NOT a silent fallback for the flagship
        # config — that path still requires the native kernel and fails
        # loudly if the extension is missing): off-spec model configs
        # (hidden != 128 or < 3 components) run the differentiable PyTorch
        # composition on rocBLAS.  Warn once per shape so a user who meant
        # to be on the hot path notices.
        key = (int(h0.shape[2]), int(h0.shape[1]))
        if key not in _WARNED_SHAPES:
            _WARNED_SHAPES.add(key)
            import warnings

            warnings.warn(
                f"fused GRU kernel supports hidden=128 and >=3 components; "
                f"got hidden={key[0]}, components={key[1]} — using the "
                f"(slower) composed rocBLAS path for this shape")
        return reference_gru_sequence(
            x_gates, w_hh, b_hh, h0, gamma, beta, reverse)
    if x_gates.is_cuda:
        dt = x_gates.dtype
        if gamma is None:
            C = h0.shape[1]
            G = x_gates.shape[-1]
            gamma = torch.ones(C, G, device=x_gates.device, dtype=dt)
            beta = torch.zeros(C, G, device=x_gates.device, dtype=dt)
        elif beta is None:
            beta = torch.zeros_like(gamma)
        args = _kernel_operands(x_gates, w_hh, b_hh, h0, gamma, beta)
        if fp8:
            # fp8 MFMA path is inference-only (BASELINE config 5): the
            # recurrent GEMM runs on e4m3 tiles, state stays fp32 in-kernel
            if torch.is_grad_enabled() and any(
                t.requires_grad for t in (x_gates, w_hh, b_hh, h0, gamma, beta)
            ):
                raise RuntimeError("fp8 GRU path does not support autograd")
            ext = require_native("fused_gru_sequence")
            h_all, _ = ext.gru_seq_forward(*args, reverse, False, True)
            return h_all
        return _FusedGRUSequence.apply(*args, reverse)
    return reference_gru_sequence(x_gates, w_hh, b_hh, h0, gamma, beta, reverse)


def fused_gru_heads(
    x_gates: torch.Tensor,       # (B, T, 3H)
    w_hh: torch.Tensor,          # (3H, H)
    b_hh: torch.Tensor,          # (3H,)
    h0: torch.Tensor,            # (B, C, H)
    gamma: torch.Tensor,         # (C, 3H)
    beta: torch.Tensor,          # (C, 3H)
    w_head: torch.Tensor,        # (O, H) head weights of this direction
    reverse: bool = False,
) -> torch.Tensor:
    """``F.linear(fused_gru_sequence(...), w_head)`` -> (B, T, C, O), with the
    head input gradient folded into the GRU backward kernel.

    On the native kernel (GPU, H == 128, C >= 3) with ``O <= 32`` this is one
    autograd node whose backward hands the O-wide ``grad_part`` straight to
    the kernel.  Everywhere else (CPU, off-spec shapes, wider heads) it is
    the differentiable composition of the two ops."""
    if not _fuses_heads(x_gates, h0, w_head):
        h_all = fused_gru_sequence(x_gates, w_hh, b_hh, h0, gamma, beta, reverse)
        return torch.nn.functional.linear(h_all, w_head.to(h_all.dtype))
    # w_head keeps its dtype so its gradient leaves the fp32 sum unrounded
    return _FusedGRUHeads.apply(
        *_kernel_operands(x_gates, w_hh, b_hh, h0, gamma, beta),
        w_head.contiguous(), reverse)


def fused_gru_decode(
    x_gates: torch.Tensor,       # (B, T, 3H)
    w_hh: torch.Tensor,          # (3H, H)
    b_hh: torch.Tensor,          # (3H,)
    h0: torch.Tensor,            # (B, C, H)
    gamma: torch.Tensor,         # (C, 3H)
    beta: torch.Tensor,          # (C, 3H)
    w_head: torch.Tensor,        # (O, H) head weights of this direction
    reverse: bool = False,
    fp8: bool = False,
    lengths: Optional[torch.Tensor] = None,   # (B,) int32 per-sample lengths
):
    """Inference decode: ``(F.linear(h_all, w_head), h_all[:, last])`` with
    ``h_all = fused_gru_sequence(...)`` -> ``out (B, T, C, O)`` and ``h_last
    (B, C, H)``, the state after the last processed step (t = T-1 forward,
    t = 0 reverse) for carrying across chunks.

    On the native kernel (GPU, H == 128, C >= 3) with ``O <= 32`` the head
    projection runs per step inside the GRU kernel and ``h_all`` is never
    materialized.  Everywhere else (CPU, off-spec shapes, wider heads) it is
    the composition of the two ops.  Not differentiable: raises when grad
    mode is on and an input requires grad.

    ``lengths`` (B,) int32 on the inputs' device, read there (no host sync):
    sample b runs its own steps t < clamp(lengths[b], 1, T) only — forward
    0..L-1, reverse L-1..0, both from h0.  ``out`` is exact zero at padded
    positions, nothing stored in padded x_gates can reach a valid output, and
    ``h_last`` is each sample's state after its own last valid step.  The
    composed path then goes through ``reference_gru_sequence`` (the plain
    sequence kernel does not know about lengths; fp8 does not apply)."""
    if torch.is_grad_enabled() and any(
        t.requires_grad
        for t in (x_gates, w_hh, b_hh, h0, gamma, beta, w_head)
    ):
        raise RuntimeError("fused_gru_decode is inference-only (no autograd)")
    if not _fuses_heads(x_gates, h0, w_head):
        if lengths is not None:
            h_all, h_last = reference_gru_sequence(
                x_gates, w_hh, b_hh, h0, gamma, beta, reverse, lengths=lengths,
                return_state=True)
        else:
            h_all = fused_gru_sequence(x_gates, w_hh, b_hh, h0, gamma, beta,
                                       reverse, fp8=fp8)
            h_last = h_all[:, 0 if reverse else -1]
        # with lengths: padded h_all rows are zero and the heads have no
        # bias, so out is zero there too
        out = torch.nn.functional.linear(h_all, w_head.to(h_all.dtype))
        return out, h_last
    ext = require_native("fused_gru_decode")
    out, h_last = ext.gru_seq_decode(
        *_kernel_operands(x_gates, w_hh, b_hh, h0, gamma, beta),
        _head_image_fwd(w_head), w_head.shape[0], bool(reverse), bool(fp8),
        lengths)
    return out, h_last
