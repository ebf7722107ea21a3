"""CPU tests of the fused dropout+residual+LayerNorm op: the Philox mask
oracle, the reference composition (the op's CPU path) and the model flag."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig, build_model_spec
from deeprest_amd.ops import (dropout_add, dropout_add_layer_norm, philox_keep_mask,
                              reference_dropout_add_layer_norm)
from deeprest_amd.ops.residual_norm import philox4x32_10


# ------------------------------------------------------------------- philox
@pytest.mark.parametrize("counter,key,expect", [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, expect):
    out = philox4x32_10(counter, key)
    assert tuple(int(o) for o in out) == expect


def test_mask_p0_keeps_everything():
    assert philox_keep_mask(1234, 7, 1000, 0.0).all()


@pytest.mark.parametrize("key", [1234, 2 ** 40 + 3])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_keep_rate(key, p):
    N = 64 * 256
    keep = philox_keep_mask(key, 7, N, p).float().mean().item()
    bound = 5 * math.sqrt(p * (1 - p) / N)
    print(f"key={key} p={p}: keep={keep:.5f} dev={abs(keep - (1 - p)):.5f} "
          f"bound={bound:.5f}")
    assert abs(keep - (1 - p)) < bound


def test_mask_depends_on_key_and_stream():
    N = 64 * 256
    base = philox_keep_mask(1234, 7, N, 0.5)
    assert not torch.equal(base, philox_keep_mask(1235, 7, N, 0.5))
    assert not torch.equal(base, philox_keep_mask(1234, 8, N, 0.5))
    assert not torch.equal(base, philox_keep_mask(1234 + 2 ** 32, 7, N, 0.5))
    assert not torch.equal(base, philox_keep_mask(1234, 7 + 2 ** 32, N, 0.5))
    assert torch.equal(base, philox_keep_mask(1234, 7, N, 0.5))


def test_mask_depends_only_on_element_index():
    a = philox_keep_mask(1234, 7, (128, 256), 0.5)
    b = philox_keep_mask(1234, 7, (8, 16, 256), 0.5)
    c = philox_keep_mask(1234, 7, 128 * 256, 0.5)
    assert a.shape == (128, 256) and b.shape == (8, 16, 256)
    assert torch.equal(a.reshape(-1), b.reshape(-1))
    assert torch.equal(a.reshape(-1), c)
    # a prefix of a longer mask, also when the length is no multiple of 4
    assert torch.equal(philox_keep_mask(1234, 7, 1001, 0.5), c[:1001])


# ------------------------------------------------------------- reference op
def test_reference_p0_matches_eager():
    torch.manual_seed(1)
    branch, residual = torch.randn(6, 5, 32), torch.randn(6, 5, 32)
    w, b = torch.randn(32), torch.randn(32)
    for training in (False, True):
        r_out, normed = reference_dropout_add_layer_norm(
            branch, residual, w, b, p=0.0, training=training)
        assert torch.equal(r_out, residual + branch)
        torch.testing.assert_close(normed, F.layer_norm(r_out, (32,), w, b),
                                   rtol=1e-6, atol=1e-6)
    # eval ignores p
    r_out, _ = dropout_add_layer_norm(branch, residual, w, b, p=0.3, training=False)
    assert torch.equal(r_out, residual + branch)
    assert torch.equal(dropout_add(branch, residual, 0.3, False), residual + branch)


def test_reference_applies_the_oracle_mask():
    torch.manual_seed(2)
    branch, residual = torch.randn(7, 24), torch.randn(7, 24)
    seed = torch.tensor([99, 5], dtype=torch.int64)
    keep = philox_keep_mask(99, 5, (7, 24), 0.5)
    r_out = dropout_add(branch, residual, 0.5, True, seed=seed)
    torch.testing.assert_close(r_out, residual + branch * keep * 2.0)
    assert 0 < keep.sum() < keep.numel()


def test_reference_gradients_flow():
    torch.manual_seed(3)
    branch = torch.randn(4, 9, 16, requires_grad=True)
    residual = torch.randn(4, 9, 16, requires_grad=True)
    w = torch.randn(16, requires_grad=True)
    b = torch.randn(16, requires_grad=True)
    seed = torch.tensor([3, 4], dtype=torch.int64)
    r_out, normed = dropout_add_layer_norm(branch, residual, w, b, 0.5, True,
                                           seed=seed)
    (r_out.sum() + (normed * torch.randn_like(normed)).sum()).backward()
    for t in (branch, residual, w, b):
        assert t.grad is not None and torch.isfinite(t.grad).all()
        assert t.grad.abs().sum() > 0
    # dropped elements pass no gradient to the branch, kept ones 1/(1-p) times
    # the residual's
    keep = philox_keep_mask(3, 4, (4, 9, 16), 0.5)
    torch.testing.assert_close(branch.grad, residual.grad * keep * 2.0)


@pytest.mark.parametrize("p", [1.0, -0.1, 1.5])
def test_p_out_of_range_raises(p):
    x = torch.randn(2, 8)
    with pytest.raises(ValueError):
        dropout_add(x, x, p, True)
    with pytest.raises(ValueError):
        dropout_add_layer_norm(x, x, torch.ones(8), torch.zeros(8), p, False)
    with pytest.raises(ValueError):
        philox_keep_mask(1, 2, 8, p)


# -------------------------------------------------------------------- model
def _tiny_spec():
    app = SyntheticApp(SyntheticAppConfig(
        n_apis=3, n_components=4, windows_per_day=30, n_days=2, seed=3))
    return build_model_spec(app.generate_featurized())


def _tiny_cfg(fused, dropout=0.0):
    return DeepRestNetConfig(d_model=32, n_heads=4, n_layers=2, d_ff=64,
                             hidden=16, comp_dim=8, dropout=dropout,
                             fused_residual_norm=fused)


def test_model_flag_equal_eval_outputs_and_keys():
    spec = _tiny_spec()
    torch.manual_seed(0)
    plain = DeepRestNet(spec, _tiny_cfg(False, dropout=0.1)).eval()
    fused = DeepRestNet(spec, _tiny_cfg(True, dropout=0.1)).eval()
    assert list(plain.state_dict().keys()) == list(fused.state_dict().keys())
    fused.load_state_dict(plain.state_dict())
    x = torch.randn(2, 12, spec.num_paths)
    with torch.no_grad():
        torch.testing.assert_close(fused(x), plain(x), rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(fused.forward_long(x, chunk_size=5),
                                   plain.forward_long(x, chunk_size=5),
                                   rtol=1e-6, atol=1e-6)


def test_flag_in_config_and_checkpoints():
    from deeprest_amd.engine.config import EngineConfig, apply_cli_overrides

    spec = _tiny_spec()
    assert DeepRestNetConfig().fused_residual_norm is False
    model = DeepRestNet(spec, _tiny_cfg(True))
    state = model.full_state()
    assert state["config"]["fused_residual_norm"] is True
    assert DeepRestNet.from_full_state(state).cfg.fused_residual_norm is True
    # a checkpoint from before the flag existed
    del state["config"]["fused_residual_norm"]
    assert DeepRestNet.from_full_state(state).cfg.fused_residual_norm is False
    cfg = apply_cli_overrides(EngineConfig(), ["model.fused_residual_norm=true"])
    assert cfg.model.fused_residual_norm is True


def _train_loss(spec, seed):
    torch.manual_seed(0)
    model = DeepRestNet(spec, _tiny_cfg(True, dropout=0.1)).train()
    x = torch.randn(4, 10, spec.num_paths)
    y = torch.rand(4, 10, spec.num_metrics)
    torch.manual_seed(seed)
    loss = model.loss(model(x), y)
    return model, loss


def test_model_training_with_dropout():
    spec = _tiny_spec()
    model, loss = _train_loss(spec, 11)
    assert torch.isfinite(loss)
    loss.backward()
    for name, prm in model.named_parameters():
        assert prm.grad is not None, name
        assert torch.isfinite(prm.grad).all(), name
    _, again = _train_loss(spec, 11)
    _, other = _train_loss(spec, 12)
    assert again.item() == loss.item()
    assert other.item() != loss.item()
