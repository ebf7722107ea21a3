"""CPU contract of ``ops.mha_packed``: it is the composition the model used to
spell out (three views of the packed projection, ``reference_mha``, the
transposing reshape), bit for bit, and gradients flow to ``qkv``."""

import pytest
import torch

from deeprest_amd.ops import attention, mha_packed, reference_mha


def _composition(qkv, n_heads):
    B, T = qkv.shape[:2]
    x = qkv.view(B, T, 3, n_heads, -1)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    return reference_mha(q, k, v).transpose(1, 2).reshape(B, T, -1)


@pytest.mark.parametrize("mode", ["auto", "off"])
@pytest.mark.parametrize("shape", [(2, 7, 3, 8), (3, 60, 8, 32), (1, 1, 1, 16)])
def test_cpu_is_the_composition_bit_for_bit(shape, mode, monkeypatch):
    B, T, H, Dh = shape
    monkeypatch.setattr(attention, "PACKED_MODE", mode)
    torch.manual_seed(0)
    qkv = torch.randn(B, T, 3 * H * Dh)
    a = qkv.clone().requires_grad_(True)
    b = qkv.clone().requires_grad_(True)
    o = mha_packed(a, H)
    o_ref = _composition(b, H)
    assert o.shape == (B, T, H * Dh)
    assert torch.equal(o, o_ref)
    g = torch.randn_like(o_ref)
    o.backward(g)
    o_ref.backward(g)
    assert a.grad is not None and torch.equal(a.grad, b.grad)
    assert a.grad[..., 2 * H * Dh:].abs().sum() > 0     # dv, non-zero at any T


def test_cpu_takes_the_5d_shape_and_a_scale():
    torch.manual_seed(1)
    qkv = torch.randn(2, 9, 3, 2, 8)
    o5 = mha_packed(qkv, 2, scale=0.3)
    o3 = mha_packed(qkv.view(2, 9, -1), 2, scale=0.3)
    assert torch.equal(o5, o3)
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    assert torch.equal(o5, reference_mha(q, k, v, 0.3).transpose(1, 2).reshape(2, 9, -1))


def test_unknown_mode_raises(monkeypatch):
    monkeypatch.setattr(attention, "PACKED_MODE", "on")
    with pytest.raises(ValueError, match="PACKED_MODE"):
        mha_packed(torch.randn(1, 2, 3 * 8), 1)


def test_model_encoder_uses_the_packed_op(monkeypatch):
    """The encoder layer hands the qkv projection to mha_packed as it comes out
    of the GEMM, (B, T, 3 * d_model) contiguous."""
    from deeprest_amd.models import net

    seen = []

    def spy(qkv, n_heads, scale=None):
        seen.append((tuple(qkv.shape), qkv.is_contiguous(), n_heads))
        return mha_packed(qkv, n_heads, scale)

    monkeypatch.setattr(net, "mha_packed", spy)
    cfg = net.DeepRestNetConfig(d_model=32, n_heads=2, n_layers=1, d_ff=64,
                                hidden=128, comp_dim=16, dropout=0.0)
    layer = net._EncoderLayer(cfg)
    x = torch.randn(2, 5, 32)
    y = layer(x)
    assert y.shape == x.shape
    assert seen == [((2, 5, 96), True, 2)]
