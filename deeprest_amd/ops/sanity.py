"""Sanity check of measured utilization against the model's quantile band —
one HIP kernel from the normalized model output to scores, debounced flags
and per-(window, metric) summaries (deeprest_amd/csrc/sanity.hip).

Band (the steps of ``Predictor.predict_tensor``, in its order), per
``(n, t, m)``: add ``base``; sort the triple; widen ``q0 = min(q0 - c, q1)``,
``q2 = max(q2 + c, q1)``; inverse-scale ``q * y_scale[m] + y_min[m]``;
``expm1`` if ``log1p``; clamp at 1e-6.

Score (the steps of ``AnomalyScorer.score``): ``band = max(q2 - q0, 1e-9)``,
``score = max((y - q2) / band, 0)``, ``over = score > threshold``, and
``flag[t]`` iff t lies in a run of at least ``min_run`` consecutive overs.

Gaps and padding: a non-finite ``measured`` value is "not observed" (the rule
of ``masked_pinball_loss``): its score is NaN, it is not over and it ends a
run.  With ``lengths``, window n is its first ``L = clamp(lengths[n], 1, T)``
positions: ``t >= L`` gets score NaN, flag 0, bands NaN, and a run ends at L.
Summaries are over the observed positions ``t < L`` only; ``max_score`` is 0
when there are none.  Both are removed by select: whatever ``out``, ``base``
or ``measured`` hold there (NaN, Inf) reaches no valid output.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .native import require_native


@dataclass
class BandScores:
    scores: torch.Tensor              # (N, T, M) float; NaN where unobserved / padded
    flags: torch.Tensor               # (N, T, M) uint8
    max_score: torch.Tensor           # (N, M) float, over observed positions (0: none)
    n_flagged: torch.Tensor           # (N, M) int32
    first_flag: torch.Tensor          # (N, M) int32, -1 if nothing is flagged
    n_observed: torch.Tensor          # (N, M) int32
    bands: Optional[torch.Tensor] = None   # (N, T, M, 3) float, on request


def _check(out, measured, y_min, y_scale, base, conformal, lengths, min_run):
    """Everything that can be wrong with a call, before any launch."""
    for name, t in (("out", out), ("measured", measured), ("y_min", y_min),
                    ("y_scale", y_scale)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
    if out.dim() != 4:
        raise ValueError(f"out must be (N, T, M, 3), got {tuple(out.shape)}")
    N, T, M, Q = out.shape
    if Q != 3:
        raise ValueError(
            f"the sanity check is defined on the quantile triple: Q must be 3, got {Q}")
    if int(min_run) < 1:
        raise ValueError(f"min_run must be >= 1, got {min_run}")
    if tuple(measured.shape) != (N, T, M):
        raise ValueError(
            f"measured must be {(N, T, M)}, got {tuple(measured.shape)}")
    for name, t in (("y_min", y_min), ("y_scale", y_scale), ("conformal", conformal)):
        if t is not None and tuple(t.shape) != (M,):
            raise ValueError(f"{name} must be ({M},), got {tuple(t.shape)}")
    if base is not None and tuple(base.shape) != (N, T, M):
        raise ValueError(f"base must be {(N, T, M)}, got {tuple(base.shape)}")
    for name, t in (("measured", measured), ("y_min", y_min), ("y_scale", y_scale),
                    ("base", base), ("conformal", conformal)):
        if t is not None and t.device != out.device:
            raise ValueError(f"{name} must be on out's device ({out.device})")
    if lengths is not None:
        if (not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int32
                or tuple(lengths.shape) != (N,) or lengths.device != out.device):
            raise ValueError(
                f"lengths must be an ({N},) int32 tensor on {out.device}")


def reference_band_scores(out: torch.Tensor, measured: torch.Tensor,
                          y_min: torch.Tensor, y_scale: torch.Tensor, *,
                          base: Optional[torch.Tensor] = None,
                          conformal: Optional[torch.Tensor] = None,
                          log1p: bool = False,
                          lengths: Optional[torch.Tensor] = None,
                          threshold: float = 0.25, min_run: int = 3,
                          want_bands: bool = False) -> BandScores:
    """Plain torch composition of the module docstring's semantics, computed
    in ``measured``'s dtype (``out`` is cast to it; float64 works).  The CPU
    path of :func:`band_scores` and the numerics oracle of the kernel."""
    _check(out, measured, y_min, y_scale, base, conformal, lengths, min_run)
    N, T, M, _ = out.shape
    dt, dev = measured.dtype, out.device
    q = out.to(dt)
    if base is not None:
        q = q + base.to(dt).unsqueeze(-1)
    q, _ = torch.sort(q, dim=-1)
    q0, q1, q2 = q.unbind(-1)
    if conformal is not None:
        c = conformal.to(dt)
        q0 = torch.minimum(q0 - c, q1)
        q2 = torch.maximum(q2 + c, q1)
    sc, mn = y_scale.to(dt), y_min.to(dt)
    q0, q1, q2 = (v * sc + mn for v in (q0, q1, q2))
    if log1p:
        q0, q1, q2 = (torch.expm1(v) for v in (q0, q1, q2))
    q0, q1, q2 = (v.clamp(min=1e-6) for v in (q0, q1, q2))
    band = (q2 - q0).clamp(min=1e-9)
    score = ((measured - q2) / band).clamp(min=0.0)

    steps = torch.arange(T, device=dev)
    if lengths is not None:
        valid = steps[None, :] < lengths.clamp(1, max(T, 1)).long()[:, None]
    else:
        valid = torch.ones(N, T, dtype=torch.bool, device=dev)
    valid = valid[:, :, None]                                  # (N, T, 1)
    obs = torch.isfinite(measured) & valid
    nan = torch.full((), float("nan"), dtype=dt, device=dev)
    zero = torch.zeros((), dtype=dt, device=dev)
    over = obs & (torch.where(obs, score, zero) > threshold)
    # the run of overs around t spans (last non-over before t, next one after)
    idx = steps[None, :, None].expand(N, T, M)
    before = torch.where(over, torch.full_like(idx, -1), idx)
    after = torch.where(over, torch.full_like(idx, T), idx)
    if T > 0:
        before = torch.cummax(before, dim=1).values
        after = torch.cummin(after.flip(1), dim=1).values.flip(1)
    flags = over & (after - before - 1 >= int(min_run))

    any_flag = flags.any(dim=1)
    first = flags.int().argmax(dim=1) if T > 0 else any_flag.long()
    res = BandScores(
        scores=torch.where(obs, score, nan),
        flags=flags.to(torch.uint8),
        max_score=(torch.where(obs, score, zero).amax(dim=1) if T > 0
                   else torch.zeros(N, M, dtype=dt, device=dev)),
        n_flagged=flags.sum(dim=1).to(torch.int32),
        first_flag=torch.where(any_flag, first, torch.full_like(first, -1)
                               ).to(torch.int32),
        n_observed=obs.sum(dim=1).to(torch.int32),
    )
    if want_bands:
        res.bands = torch.where(valid.unsqueeze(-1).expand(N, T, M, 3),
                                torch.stack((q0, q1, q2), dim=-1), nan)
    return res


def band_scores(out: torch.Tensor, measured: torch.Tensor,
                y_min: torch.Tensor, y_scale: torch.Tensor, *,
                base: Optional[torch.Tensor] = None,
                conformal: Optional[torch.Tensor] = None,
                log1p: bool = False,
                lengths: Optional[torch.Tensor] = None,
                threshold: float = 0.25, min_run: int = 3,
                want_bands: bool = False) -> BandScores:
    """out: (N, T, M, 3) normalized model output, f32 or bf16; measured:
    (N, T, M) raw units; y_min / y_scale: (M,) per-metric scaler (scale 1,
    min 0 for a scaler that leaves its metric alone); base: optional
    (N, T, M) ridge residual base; conformal: optional (M,); lengths: optional
    (N,) int32 on out's device, read there and clamped to [1, T].

    On a GPU this is the HIP kernel (f32 operands; no eager fallback), on CPU
    :func:`reference_band_scores`."""
    _check(out, measured, y_min, y_scale, base, conformal, lengths, min_run)
    if not out.is_cuda:
        return reference_band_scores(
            out, measured, y_min, y_scale, base=base, conformal=conformal,
            log1p=log1p, lengths=lengths, threshold=threshold, min_run=min_run,
            want_bands=want_bands)
    ext = require_native("band_scores")
    if out.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"out must be f32 or bf16 on a GPU, got {out.dtype}")
    f32 = lambda t: None if t is None else t.float().contiguous()
    got = ext.band_scores(out.contiguous(), f32(measured), f32(y_min),
                          f32(y_scale), f32(base), f32(conformal), bool(log1p),
                          None if lengths is None else lengths.contiguous(),
                          float(threshold), int(min_run),
                          bool(want_bands))
    return BandScores(*got[:6], bands=got[6] if want_bands else None)
