"""DeepRestNet — the MI355X-native estimation engine.

Architecture (the north star's re-design of the reference QuantileRNN,
reference: resource-estimation/qrnn.py:6-56):

  traffic (B, T, P call-path counts)
    -> input projection (P -> D)                      [rocBLAS GEMM]
    -> attention traffic encoder, n_layers x
         pre-LN MHA over the T axis + FFN            [HIP MHA + LayerNorm
                                                       kernels, rocBLAS GEMMs]
    -> call-graph propagation over the component
       graph (mean-aggregate neighbor embeddings)    [small GEMMs]
    -> per-component FiLM-conditioned GRU decoders   [fused HIP GRU sequence
       over time (optionally bidirectional)           kernel — the hot op]
    -> per-resource-type quantile heads (H -> Q)     [small GEMMs]
  output: (B, T, M, Q) quantile predictions for every component_resource
          metric, Q = (.05, .50, .95)

Where the reference runs one bidirectional GRU per metric and mixes experts
by averaging all other experts' outputs (qrnn.py:46-53, O(M^2) in metrics),
this design shares one encoder, conditions a shared recurrent decoder per
*component* via FiLM, and propagates information along the actual
application call graph — O(M), and every stage maps onto MFMA-shaped
compute.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..data.featurize import FeaturizedData
from ..ops import (dropout_add, dropout_add_layer_norm, fused_gru_decode,
                   fused_gru_heads, fused_gru_sequence, layer_norm,
                   masked_pinball_loss, mha_forward, mha_packed, pinball_loss)
from ..ops.gru import HEAD_FUSE_MAX_OUT, gru_kernel_supports
from ..ops.linear_bigk import bigk_linear


# --------------------------------------------------------------------- spec
@dataclass
class ModelSpec:
    """Static application structure the model is built around."""

    num_paths: int
    components: List[str]                 # decoder index -> component name
    resources: List[str]                  # head index -> resource type
    metric_names: List[str]               # output order (dataset order)
    comp_of: List[int]                    # metric -> component index
    res_of: List[int]                     # metric -> resource-type index
    adjacency: np.ndarray                 # (C, C) row-normalized call graph

    @property
    def num_components(self) -> int:
        return len(self.components)

    @property
    def num_metrics(self) -> int:
        return len(self.metric_names)


def _split_metric_ident(ident: str, known_components: Sequence[str]) -> Tuple[str, str]:
    """component_resource -> (component, resource), robust to '_' in names."""
    best = None
    for comp in known_components:
        if ident.startswith(comp + "_") and (best is None or len(comp) > len(best)):
            best = comp
    if best is not None:
        return best, ident[len(best) + 1 :]
    comp, _, res = ident.rpartition("_")
    return comp, res


def build_model_spec(data: FeaturizedData) -> ModelSpec:
    """Derive the static structure (components, resources, call graph)."""
    known = [c for c in data.invocations.keys() if c != "general"]
    comps: List[str] = []
    ress: List[str] = []
    comp_of: List[int] = []
    res_of: List[int] = []
    for ident in data.metric_names:
        if ident in data.resource_components:
            comp = data.resource_components[ident]
            res = ident[len(comp) + 1 :]
        else:
            comp, res = _split_metric_ident(ident, known)
        if comp not in comps:
            comps.append(comp)
        if res not in ress:
            ress.append(res)
        comp_of.append(comps.index(comp))
        res_of.append(ress.index(res))

    C = len(comps)
    A = np.eye(C, dtype=np.float64)
    if data.feature_space is not None:
        cidx = {c: i for i, c in enumerate(comps)}
        for path in data.feature_space.paths:
            if len(path) < 2:
                continue
            parent_comp = path[-2][0]
            child_comp = path[-1][0]
            pi, ci = cidx.get(parent_comp), cidx.get(child_comp)
            if pi is not None and ci is not None and pi != ci:
                A[pi, ci] = 1.0
                A[ci, pi] = 1.0
    A = A / A.sum(axis=1, keepdims=True)
    return ModelSpec(
        num_paths=data.num_paths,
        components=comps,
        resources=ress,
        metric_names=list(data.metric_names),
        comp_of=comp_of,
        res_of=res_of,
        adjacency=A,
    )


# ------------------------------------------------------------------- config
@dataclass
class DeepRestNetConfig:
    d_model: int = 256
    n_heads: int = 8
    n_layers: int = 2
    d_ff: int = 512
    hidden: int = 128                     # GRU hidden size
    comp_dim: int = 64                    # component embedding size
    quantiles: Tuple[float, ...] = (0.05, 0.50, 0.95)
    dropout: float = 0.1
    bidirectional: bool = True
    prop_rounds: int = 2                  # call-graph propagation rounds
    fp8_inference: bool = False           # fp8 MFMA GRU decode at eval time
    linear_bias: bool = False             # biases on encoder/x_proj Linears:
                                          # biasless default (LayerNorms and
                                          # metric_bias absorb shifts) saves
                                          # ~1.1 ms/step of bias-grad
                                          # reductions at accuracy parity
                                          # (profiles/r02_perf_notes.md)
    fused_residual_norm: bool = False     # encoder residual glue (dropout +
                                          # add + the following LayerNorm) as
                                          # one kernel with an in-kernel
                                          # Philox mask; same parameters and
                                          # state_dict keys in both modes
    fused_head_grad: bool = True          # decoder + quantile heads as one
                                          # autograd node per direction: the
                                          # GRU backward kernel forms the head
                                          # input gradient from the Q-wide head
                                          # gradient itself (no (B,T,C,H)
                                          # round trip); applies when the
                                          # native GRU kernel runs and head
                                          # dropout is inactive; same
                                          # parameters and state_dict keys
    fused_head_decode: bool = False       # inference (eval, no grad, GPU):
                                          # decoder + quantile heads as one
                                          # kernel per direction that never
                                          # writes the (B,T,C,H) hidden
                                          # sequence; forward_long then keeps
                                          # only head-wide outputs per chunk;
                                          # same parameters and state_dict keys

    def to_dict(self) -> dict:
        return {
            "d_model": self.d_model, "n_heads": self.n_heads,
            "n_layers": self.n_layers, "d_ff": self.d_ff,
            "hidden": self.hidden, "comp_dim": self.comp_dim,
            "quantiles": tuple(self.quantiles), "dropout": self.dropout,
            "bidirectional": self.bidirectional, "prop_rounds": self.prop_rounds,
            "fp8_inference": self.fp8_inference, "linear_bias": self.linear_bias,
            "fused_residual_norm": self.fused_residual_norm,
            "fused_head_grad": self.fused_head_grad,
            "fused_head_decode": self.fused_head_decode,
        }


# ------------------------------------------------------------------ modules
class _LayerNormOp(nn.Module):
    """nn.LayerNorm replacement routed through the HIP kernel on GPU."""

    def __init__(self, dim: int, eps: float = 1e-5) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))
        self.eps = eps

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return layer_norm(x, self.weight, self.bias, self.eps)


class _EncoderLayer(nn.Module):
    def __init__(self, cfg: DeepRestNetConfig) -> None:
        super().__init__()
        d = cfg.d_model
        self.ln1 = _LayerNormOp(d)
        self.ln2 = _LayerNormOp(d)
        lb = cfg.linear_bias
        self.qkv = nn.Linear(d, 3 * d, bias=lb)
        self.proj = nn.Linear(d, d, bias=lb)
        self.ff1 = nn.Linear(d, cfg.d_ff, bias=lb)
        self.ff2 = nn.Linear(cfg.d_ff, d, bias=lb)
        self.n_heads = cfg.n_heads
        self.dropout = nn.Dropout(cfg.dropout)

    def _attention(self, h: torch.Tensor,
                   kv_lengths: Optional[torch.Tensor]) -> torch.Tensor:
        """(B, T, D) normed input -> (B, T, D) attention output, before proj."""
        if kv_lengths is None:
            return mha_packed(self.qkv(h), self.n_heads)
        # per-sample lengths (inference only): the (B, H, T, Dh) kernel
        B, T, D = h.shape
        qkv = self.qkv(h).view(B, T, 3, self.n_heads, D // self.n_heads)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))  # (B,h,T,dh)
        attn = mha_forward(q, k, v, kv_lengths=kv_lengths)
        return attn.transpose(1, 2).reshape(B, T, D)

    def forward(self, x: torch.Tensor,
                kv_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        B, T, D = x.shape
        h = self.ln1(x)
        attn = self._attention(h, kv_lengths)
        x = x + self.dropout(self.proj(attn))
        h = self.ln2(x)
        x = x + self.dropout(self.ff2(F.gelu(self.ff1(h))))
        return x

    def forward_fused(self, x: torch.Tensor, h: torch.Tensor,
                      next_ln: Optional[_LayerNormOp],
                      kv_lengths: Optional[torch.Tensor] = None):
        """Same math with the residual glue fused: takes the residual stream
        ``x`` and ``h = ln1(x)``; the FFN residual add is fused with the NEXT
        layer's ln1 (``next_ln``; None for the last layer).  Returns
        ``(x, next_ln(x))`` — the second entry is None for the last layer."""
        B, T, D = x.shape
        p, training = self.dropout.p, self.training
        attn = self._attention(h, kv_lengths)
        x, h = dropout_add_layer_norm(self.proj(attn), x, self.ln2.weight,
                                      self.ln2.bias, p, training, self.ln2.eps)
        ff = self.ff2(F.gelu(self.ff1(h)))
        if next_ln is None:
            return dropout_add(ff, x, p, training), None
        return dropout_add_layer_norm(ff, x, next_ln.weight, next_ln.bias, p,
                                      training, next_ln.eps)


class _GraphPropagation(nn.Module):
    """Mean-aggregate message passing over the application call graph."""

    def __init__(self, cfg: DeepRestNetConfig, num_components: int,
                 adjacency: np.ndarray) -> None:
        super().__init__()
        self.emb = nn.Parameter(torch.randn(num_components, cfg.comp_dim) * 0.02)
        self.w_self = nn.ModuleList(
            [nn.Linear(cfg.comp_dim, cfg.comp_dim) for _ in range(cfg.prop_rounds)]
        )
        self.w_nbr = nn.ModuleList(
            [nn.Linear(cfg.comp_dim, cfg.comp_dim) for _ in range(cfg.prop_rounds)]
        )
        self.register_buffer(
            "adj", torch.from_numpy(np.asarray(adjacency, dtype=np.float32))
        )

    def forward(self) -> torch.Tensor:
        e = self.emb
        for ws, wn in zip(self.w_self, self.w_nbr):
            e = F.relu(ws(e) + wn(self.adj @ e))
        return e                                               # (C, comp_dim)


class _GRUDecoderBank(nn.Module):
    """Shared-weight, per-component FiLM-conditioned GRU over time."""

    def __init__(self, cfg: DeepRestNetConfig, num_components: int) -> None:
        super().__init__()
        H = cfg.hidden
        D = cfg.d_model
        self.hidden = H
        self.bidirectional = cfg.bidirectional
        self.x_proj = nn.Linear(D, 3 * H, bias=cfg.linear_bias)
        self.w_hh = nn.Parameter(torch.empty(3 * H, H))
        self.b_hh = nn.Parameter(torch.zeros(3 * H))
        self.cond_gamma = nn.Linear(cfg.comp_dim, 3 * H)
        self.cond_beta = nn.Linear(cfg.comp_dim, 3 * H)
        self.h0_proj = nn.Linear(cfg.comp_dim, H)
        if cfg.bidirectional:
            self.x_proj_r = nn.Linear(D, 3 * H, bias=cfg.linear_bias)
            self.w_hh_r = nn.Parameter(torch.empty(3 * H, H))
            self.b_hh_r = nn.Parameter(torch.zeros(3 * H))
            self.cond_gamma_r = nn.Linear(cfg.comp_dim, 3 * H)
            self.cond_beta_r = nn.Linear(cfg.comp_dim, 3 * H)
            self.h0_proj_r = nn.Linear(cfg.comp_dim, H)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        stdv = 1.0 / (self.hidden ** 0.5)
        with torch.no_grad():
            self.w_hh.uniform_(-stdv, stdv)
            if self.bidirectional:
                self.w_hh_r.uniform_(-stdv, stdv)
            # FiLM starts as identity: gamma ~ 1, beta ~ 0
            for g in (self.cond_gamma, getattr(self, "cond_gamma_r", None)):
                if g is not None:
                    g.weight.mul_(0.1)
                    g.bias.fill_(1.0)
            for b in (self.cond_beta, getattr(self, "cond_beta_r", None)):
                if b is not None:
                    b.weight.mul_(0.1)
                    b.bias.zero_()

    @property
    def dirs(self) -> int:
        return 2 if self.bidirectional else 1

    def _of(self, name: str, d: int):
        """Direction d's parameter or sub-module: the reverse direction's
        carry the suffix "_r"."""
        return getattr(self, name + ("_r" if d else ""))

    def x_gates(self, enc: torch.Tensor, d: int) -> torch.Tensor:
        return self._of("x_proj", d)(enc)                      # (B, T, 3H)

    def film(self, comp: torch.Tensor, d: int):
        """Direction d's FiLM condition (gamma, beta), each (C, 3H)."""
        return self._of("cond_gamma", d)(comp), self._of("cond_beta", d)(comp)

    def h0(self, comp: torch.Tensor, B: int, d: int) -> torch.Tensor:
        """Direction d's initial state (B, C, H), contiguous."""
        h0 = torch.tanh(self._of("h0_proj", d)(comp))
        return h0.unsqueeze(0).expand(B, comp.shape[0], self.hidden).contiguous()

    def operands(self, enc: torch.Tensor, comp: torch.Tensor, d: int):
        """Direction d's ``(x_gates, w_hh, b_hh, h0, gamma, beta)``, the
        leading arguments of the fused GRU ops."""
        xg = self.x_gates(enc, d)
        gamma, beta = self.film(comp, d)
        return (xg, self._of("w_hh", d), self._of("b_hh", d),
                self.h0(comp, enc.shape[0], d), gamma, beta)

    def forward(self, enc: torch.Tensor, comp: torch.Tensor, fp8: bool = False):
        """enc: (B, T, D); comp: (C, comp_dim) -> tuple of direction outputs
        (each (B, T, C, H)); the heads consume the halves separately so no
        concat copy is ever materialized."""
        return tuple(
            fused_gru_sequence(*self.operands(enc, comp, d), reverse=bool(d),
                               fp8=fp8)
            for d in range(self.dirs))

    def forward_heads(self, enc: torch.Tensor, comp: torch.Tensor,
                      w_heads: Sequence[torch.Tensor]) -> torch.Tensor:
        """Decoder and head projection as one op per direction
        (ops.fused_gru_heads): ``w_heads[d]`` is direction d's (O, H) head
        weight slice; returns the summed head output (B, T, C, O).  Same
        math as ``forward`` followed by a per-direction linear."""
        out = None
        for d in range(self.dirs):
            part = fused_gru_heads(*self.operands(enc, comp, d), w_heads[d],
                                   reverse=bool(d))
            out = part if out is None else out + part
        return out

    def decode_heads(self, enc: torch.Tensor, comp: torch.Tensor,
                     w_heads: Sequence[torch.Tensor], fp8: bool = False,
                     d: int = 0, lengths: Optional[torch.Tensor] = None):
        """Inference decode of direction ``d`` (ops.fused_gru_decode):
        returns ``(part (B, T, C, O), h_last (B, C, H))`` with ``part`` that
        direction's head output; the hidden sequence is never materialized.
        ``lengths`` (B,) int32: per-sample window lengths, see the op."""
        return fused_gru_decode(*self.operands(enc, comp, d), w_heads[d],
                                reverse=bool(d), fp8=fp8, lengths=lengths)


# -------------------------------------------------------------------- model
class DeepRestNet(nn.Module):
    def __init__(self, spec: ModelSpec, cfg: Optional[DeepRestNetConfig] = None) -> None:
        super().__init__()
        self.spec = spec
        self.cfg = cfg or DeepRestNetConfig()
        cfg = self.cfg

        # in_norm immediately re-centers, so the in_proj bias is redundant
        # when biasless mode is on
        self.in_proj = nn.Linear(spec.num_paths, cfg.d_model,
                                 bias=cfg.linear_bias)
        self.in_norm = _LayerNormOp(cfg.d_model)
        self.layers = nn.ModuleList([_EncoderLayer(cfg) for _ in range(cfg.n_layers)])
        self.graph = _GraphPropagation(cfg, spec.num_components, spec.adjacency)
        self.decoder = _GRUDecoderBank(cfg, spec.num_components)
        self.dropout = nn.Dropout(cfg.dropout)

        dirs = 2 if cfg.bidirectional else 1
        Q = len(cfg.quantiles)
        # bias=False: metric_bias below subsumes it, and the per-head bias
        # gradient was a pathological 28M->9 reduction on the GPU
        self.heads = nn.ModuleList(
            [nn.Linear(cfg.hidden * dirs, Q, bias=False)
             for _ in range(len(spec.resources))]
        )
        self.metric_bias = nn.Parameter(torch.zeros(spec.num_metrics, Q))
        self.register_buffer("comp_of", torch.tensor(spec.comp_of, dtype=torch.long))
        self.register_buffer("res_of", torch.tensor(spec.res_of, dtype=torch.long))
        # fast path: when the metric order IS (component-major x resource) the
        # per-metric gather is a plain reshape (true for the synthetic apps;
        # avoids an indexing_backward scatter over ~10^6 rows)
        C, R, M = spec.num_components, len(spec.resources), spec.num_metrics
        grid_c = [c for c in range(C) for _ in range(R)]
        grid_r = list(range(R)) * C
        self._gather_is_reshape = (M == C * R and spec.comp_of == grid_c
                                   and spec.res_of == grid_r)

        # positional encoding over the window (sinusoidal, not learned: windows
        # slide, so absolute position has no meaning beyond phase)
        self._pos_cache: Optional[torch.Tensor] = None

    def _pos_encoding(self, T: int, device, dtype) -> torch.Tensor:
        c = self._pos_cache
        if c is not None and c.shape[0] >= T and c.device == device:
            return c[:T].to(dtype)
        D = self.cfg.d_model
        pos = torch.arange(T, device=device, dtype=torch.float32).unsqueeze(1)
        i = torch.arange(0, D, 2, device=device, dtype=torch.float32)
        div = torch.exp(-np.log(10000.0) * i / D)
        pe = torch.zeros(T, D, device=device)
        pe[:, 0::2] = torch.sin(pos * div)
        pe[:, 1::2] = torch.cos(pos * div)
        self._pos_cache = pe
        return pe.to(dtype)

    def forward(self, traffic: torch.Tensor,
                lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """traffic: (B, T, P) normalized call-path counts -> (B, T, M, Q).

        ``lengths`` (B,) int32 on traffic's device (inference only: eval
        mode, grad disabled): sample b is the window traffic[b, :lengths[b]]
        and everything behind it is padding.  ``out[b, :L]`` is what the
        model returns for that window alone, nothing stored in the padding
        can reach it, and ``out[b, L:]`` is exact zero.  The lengths are
        read on the device only, so a captured graph stays valid when the
        buffer is rewritten between replays.  With lengths every stage but
        two is per-position; attention masks the padded keys and the decoders
        run each sample's own steps (both inside their kernels on GPU)."""
        B, T, P = traffic.shape
        if lengths is not None:
            if self.training or torch.is_grad_enabled():
                raise ValueError(
                    "lengths are inference-only: call model.eval() and run "
                    "under torch.no_grad()")
            if lengths.dim() != 1 or lengths.shape[0] != B:
                raise ValueError(
                    f"lengths must be ({B},), got {tuple(lengths.shape)}")
            lengths = lengths.to(device=traffic.device, dtype=torch.int32)
        x = self._encode(traffic, lengths)
        comp = self.graph()                                   # (C, comp_dim)
        fp8 = (self.cfg.fp8_inference and not self.training
               and traffic.is_cuda and not torch.is_grad_enabled())
        # with lengths always the decode op, whatever cfg.fused_head_decode
        # says: it is the GRU entry that knows about lengths (native kernel
        # on GPU when the shape fits it, the composed reference otherwise)
        if lengths is not None or self._use_head_decode(x, comp):
            preds = self._finish_heads(self._decode_sum(x, comp, fp8, lengths))
            if lengths is None:
                return preds
            # metric_bias made the padded positions non-zero: zero them by
            # select
            valid = (torch.arange(T, device=preds.device)[None, :]
                     < lengths.clamp(1, T)[:, None])
            return torch.where(valid[:, :, None, None], preds,
                               torch.zeros((), dtype=preds.dtype,
                                           device=preds.device))
        if self._use_fused_heads(x, comp, fp8):
            return self._finish_heads(self.decoder.forward_heads(
                x, comp, self._head_weights_per_dir()))
        h_dirs = self.decoder(x, comp, fp8=fp8)               # tuple of (B,T,C,H)
        return self._apply_heads(h_dirs)

    def _encode(self, traffic: torch.Tensor,
                lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """traffic (B, T, P) -> encoder output (B, T, D); ``lengths`` as in
        forward()."""
        x = self.in_proj(traffic)
        x = x + self._pos_encoding(x.shape[1], x.device, x.dtype)
        x = self.in_norm(x)
        if self.cfg.fused_residual_norm:
            return self._encode_fused(x, lengths)
        for layer in self.layers:
            x = layer(x, lengths)
        return x

    def _decode_sum(self, enc: torch.Tensor, comp: torch.Tensor, fp8: bool,
                    lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Sum over directions of the decode op's head outputs (B, T, C, R*Q)."""
        w_dirs = self._head_weights_per_dir()
        out = None
        for d in range(len(w_dirs)):
            part, _ = self.decoder.decode_heads(enc, comp, w_dirs, fp8, d, lengths)
            out = part if out is None else out + part
        return out

    def _native_heads_fit(self, enc: torch.Tensor, comp: torch.Tensor) -> bool:
        """GPU input, the decoder runs the native GRU kernel, and all heads
        together fit its head phase: one K=32 MFMA step in the backward, two
        16-wide output tiles in the decode."""
        return (enc.is_cuda
                and gru_kernel_supports(self.cfg.hidden, comp.shape[0])
                and len(self.heads) * len(self.cfg.quantiles) <= HEAD_FUSE_MAX_OUT)

    def _use_fused_heads(self, enc: torch.Tensor, comp: torch.Tensor,
                         fp8: bool) -> bool:
        """cfg.fused_head_grad applies when the native kernel does (not its
        fp8 inference variant) and the head dropout is the identity."""
        if not self.cfg.fused_head_grad or fp8:
            return False
        if self.training and self.dropout.p > 0:
            return False
        return self._native_heads_fit(enc, comp)

    def _use_head_decode(self, enc: torch.Tensor, comp: torch.Tensor) -> bool:
        """cfg.fused_head_decode applies to inference only — eval mode, grad
        disabled — when the native kernel does."""
        if not self.cfg.fused_head_decode or self.training:
            return False
        return not torch.is_grad_enabled() and self._native_heads_fit(enc, comp)

    def _head_weight_of_dir(self, w_all: torch.Tensor, d: int) -> torch.Tensor:
        """Direction d's contiguous (R*Q, H) slice of the concatenated head
        weights."""
        H = self.cfg.hidden
        return w_all[:, d * H : (d + 1) * H].contiguous()

    def _head_weights_per_dir(self) -> List[torch.Tensor]:
        w_all = self._head_weights()
        return [self._head_weight_of_dir(w_all, d)
                for d in range(self.decoder.dirs)]

    def _encode_fused(self, x: torch.Tensor,
                      kv_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Encoder stack with cfg.fused_residual_norm: carries the residual
        stream ``x`` and the normed tensor ``h`` the next sub-block consumes,
        so every ``x + dropout(branch)`` and the LayerNorm after it are one
        kernel.  Layer 0's ln1 has no residual add in front of it and is the
        plain layer_norm; the last FFN add has no LayerNorm behind it."""
        n = len(self.layers)
        if n == 0:
            return x
        h = self.layers[0].ln1(x)
        for i, layer in enumerate(self.layers):
            next_ln = self.layers[i + 1].ln1 if i + 1 < n else None
            x, h = layer.forward_fused(x, h, next_ln, kv_lengths)
        return x

    def _apply_heads(self, h_dirs) -> torch.Tensor:
        """Per-resource heads as a sum of per-direction GEMMs (no concat),
        each with a batched-K backward (ops/linear_bigk.py)."""
        w_all = self._head_weights()
        out = None
        for d, h_d in enumerate(h_dirs):
            h_d = self.dropout(h_d)
            part = bigk_linear(h_d, self._head_weight_of_dir(w_all, d))
            out = part if out is None else out + part
        return self._finish_heads(out)

    def _head_weights(self) -> torch.Tensor:
        return torch.cat([h.weight for h in self.heads], dim=0)    # (R*Q, H*dirs)

    def _finish_heads(self, out: torch.Tensor) -> torch.Tensor:
        """(B, T, C, R*Q) summed head outputs -> (B, T, M, Q) predictions."""
        B, T, C = out.shape[0], out.shape[1], out.shape[2]
        R = len(self.heads)
        Q = len(self.cfg.quantiles)
        outs = out.view(B, T, C, R, Q)
        if self._gather_is_reshape:
            preds = outs.reshape(B, T, C * R, Q)
        else:
            preds = outs[:, :, self.comp_of, self.res_of, :]  # (B, T, M, Q)
        return preds + self.metric_bias

    def loss(self, outputs: torch.Tensor, labels: torch.Tensor,
             missing: bool = False) -> torch.Tensor:
        """``missing=True``: NaN labels are "not observed" and the loss is the
        mean of per-metric means over the observed entries."""
        if missing:
            return masked_pinball_loss(outputs, labels, self.cfg.quantiles)
        return pinball_loss(outputs, labels, self.cfg.quantiles)

    # -------------------------------------------------- long-horizon path
    @torch.no_grad()
    def forward_long(self, traffic: torch.Tensor, chunk_size: int = 4096) -> torch.Tensor:
        """Streaming inference over arbitrarily long horizons (SURVEY.md 5.7,
        BASELINE config 5: 7-day@1s ~ 604,800 steps).

        The encoder attends within chunks (attention cost stays
        O(chunk^2) per chunk); the GRU decoders carry hidden state across
        chunk boundaries — a forward sweep left->right and, when
        bidirectional, a reverse sweep right->left — so recurrence is exact
        over the whole horizon while peak memory is O(chunk).

        Without cfg.fused_head_decode every chunk's (B, Tc, C, H) hidden
        sequence is kept per direction until the heads run at the end; with
        it (GPU, eval mode) each chunk keeps only its (B, Tc, C, R*Q) head
        output and the carried state.

        traffic: (B, T_total, P) -> (B, T_total, M, Q)
        """
        B, T_total, P = traffic.shape
        cfg = self.cfg
        dec = self.decoder
        comp = self.graph()

        bounds = list(range(0, T_total, chunk_size)) + [T_total]
        chunks = list(zip(bounds[:-1], bounds[1:]))

        # fp8 MFMA decode (BASELINE config 5) applies to the long-horizon
        # path exactly as to forward()
        fp8 = bool(cfg.fp8_inference and traffic.is_cuda)
        # head decode inside the GRU kernel: per chunk only the head-wide
        # part and the carried state survive
        use_dec = self._use_head_decode(traffic, comp)
        w_dirs = self._head_weights_per_dir() if use_dec else None

        enc_cache = [None] * len(chunks)

        def sweep(d):
            """Direction d over all chunks, left->right for d = 0 (encoding
            each chunk on the way) and right->left for d = 1, the state
            carried from chunk to chunk; returns the per-chunk outputs."""
            # launch order kept stable: the forward sweep builds its initial
            # state before the FiLM pair, the reverse sweep after it
            if d == 0:
                h = dec.h0(comp, B, d).to(traffic.dtype)
            gamma, beta = dec.film(comp, d)
            if d == 1:
                h = dec.h0(comp, B, d).to(traffic.dtype)
            w_hh, b_hh = dec._of("w_hh", d), dec._of("b_hh", d)
            outs = [None] * len(chunks)
            for ci in (reversed(range(len(chunks))) if d else range(len(chunks))):
                if enc_cache[ci] is None:
                    s, e = chunks[ci]
                    enc_cache[ci] = self._encode(traffic[:, s:e])
                xg = dec.x_gates(enc_cache[ci], d)
                if use_dec:
                    outs[ci], h = fused_gru_decode(xg, w_hh, b_hh, h, gamma, beta,
                                                   w_dirs[d], reverse=bool(d),
                                                   fp8=fp8)
                    continue
                outs[ci] = fused_gru_sequence(xg, w_hh, b_hh, h, gamma, beta,
                                              reverse=bool(d), fp8=fp8)
                h = outs[ci][:, 0 if d else -1].contiguous()
            return outs

        h_chunks = list(zip(*[sweep(d) for d in range(dec.dirs)]))

        if use_dec:
            preds = [self._finish_heads(sum(parts[1:], parts[0]))
                     for parts in h_chunks]
            return torch.cat(preds, dim=1)
        preds = [self._apply_heads(h_dirs) for h_dirs in h_chunks]
        return torch.cat(preds, dim=1)

    # ---- checkpoint helpers (spec travels with the weights) ----
    def full_state(self) -> dict:
        return {
            "state_dict": self.state_dict(),
            "config": self.cfg.to_dict(),
            "spec": {
                "num_paths": self.spec.num_paths,
                "components": self.spec.components,
                "resources": self.spec.resources,
                "metric_names": self.spec.metric_names,
                "comp_of": self.spec.comp_of,
                "res_of": self.spec.res_of,
                "adjacency": self.spec.adjacency,
            },
        }

    @staticmethod
    def from_full_state(state: dict) -> "DeepRestNet":
        spec = ModelSpec(**state["spec"])
        config = dict(state["config"])
        # checkpoints from before the biasless default carried biases
        config.setdefault("linear_bias", True)
        cfg = DeepRestNetConfig(**config)
        model = DeepRestNet(spec, cfg)
        model.load_state_dict(state["state_dict"])
        return model
