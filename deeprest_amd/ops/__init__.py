"""Compute ops for the estimation engine.

Every hot op has two implementations:

- a hand-written CDNA4 HIP kernel (deeprest_amd/csrc/*.hip, built in-tree as
  ``deeprest_amd._C``) — the ONLY path used on a GPU;
- a plain PyTorch composition (``reference_*``) used on CPU for tests and as
  the numerics oracle the kernels are validated against.

On a CUDA (ROCm) tensor these ops refuse to fall back: if the native
extension is missing on a GPU machine they raise, so a silent eager fallback
can never masquerade as kernel coverage.
"""

from .native import native_available, require_native, load_native
from .gru import (fused_gru_decode, fused_gru_heads, fused_gru_sequence,
                  reference_gru_sequence)
from .layernorm import layer_norm, reference_layer_norm
from .residual_norm import (dropout_add, dropout_add_layer_norm, philox_keep_mask,
                            reference_dropout_add_layer_norm)
from .attention import mha_forward, mha_packed, reference_mha, reference_mha_step
from .pinball import (masked_pinball_loss, pinball_loss,
                      reference_masked_pinball_loss, reference_pinball_loss)
from .adam import fused_adam_step, reference_adam_step
from .sanity import BandScores, band_scores, reference_band_scores

__all__ = [
    "native_available",
    "require_native",
    "load_native",
    "fused_gru_sequence",
    "fused_gru_heads",
    "fused_gru_decode",
    "reference_gru_sequence",
    "layer_norm",
    "reference_layer_norm",
    "dropout_add",
    "dropout_add_layer_norm",
    "philox_keep_mask",
    "reference_dropout_add_layer_norm",
    "mha_forward",
    "mha_packed",
    "reference_mha",
    "reference_mha_step",
    "pinball_loss",
    "reference_pinball_loss",
    "masked_pinball_loss",
    "reference_masked_pinball_loss",
    "fused_adam_step",
    "reference_adam_step",
    "BandScores",
    "band_scores",
    "reference_band_scores",
]
