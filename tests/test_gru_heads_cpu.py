"""CPU tests of the GRU + quantile-head op (ops.fused_gru_heads) and of the
model flag that routes the decoder through it (cfg.fused_head_grad).

Off the native kernel the op is the differentiable composition of
reference_gru_sequence and F.linear, so everything here is exact up to fp32
reassociation."""

import pytest
import torch
import torch.nn.functional as F

from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig, build_model_spec
from deeprest_amd.ops import fused_gru_heads, reference_gru_sequence

NAMES = ["x_gates", "w_hh", "b_hh", "h0", "gamma", "beta", "w_head"]


def _op_inputs(B, T, C, H, O, seed=0):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=gen) * 0.4
    return [mk(B, T, 3 * H), mk(3 * H, H) / H ** 0.5, mk(3 * H) * 0.2,
            mk(B, C, H), 1.0 + 0.1 * mk(C, 3 * H), 0.1 * mk(C, 3 * H),
            mk(O, H) / H ** 0.5], mk(B, T, C, O)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 4, 128, 9), (3, 4, 2, 16, 6),
                                   (2, 3, 3, 128, 33)])
def test_reference_path_is_gru_then_linear(shape, reverse):
    B, T, C, H, O = shape
    ins, grad = _op_inputs(B, T, C, H, O)
    a = [t.clone().requires_grad_(True) for t in ins]
    b = [t.clone().requires_grad_(True) for t in ins]
    out = fused_gru_heads(*a, reverse=reverse)
    ref = F.linear(reference_gru_sequence(*b[:6], reverse=reverse), b[6])
    assert out.shape == (B, T, C, O)
    torch.testing.assert_close(out, ref, rtol=1e-6, atol=1e-6)
    out.backward(grad)
    ref.backward(grad)
    for name, ta, tb in zip(NAMES, a, b):
        assert ta.grad is not None, name
        torch.testing.assert_close(ta.grad, tb.grad, rtol=1e-5, atol=1e-6,
                                   msg=lambda m, n=name: f"{n}: {m}")


# -------------------------------------------------------------------- model
def _tiny_spec():
    app = SyntheticApp(SyntheticAppConfig(
        n_apis=3, n_components=4, windows_per_day=30, n_days=2, seed=3))
    return build_model_spec(app.generate_featurized())


def _tiny_cfg(fused, dropout=0.0):
    return DeepRestNetConfig(d_model=32, n_heads=4, n_layers=1, d_ff=64,
                             hidden=16, comp_dim=8, dropout=dropout,
                             fused_head_grad=fused)


def test_model_flag_same_outputs_gradients_and_keys():
    spec = _tiny_spec()
    torch.manual_seed(0)
    off = DeepRestNet(spec, _tiny_cfg(False))
    on = DeepRestNet(spec, _tiny_cfg(True))
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    assert ([n for n, _ in on.named_parameters()]
            == [n for n, _ in off.named_parameters()])
    on.load_state_dict(off.state_dict())
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(2, 12, spec.num_paths, generator=gen)
    y = torch.rand(2, 12, spec.num_metrics, generator=gen)
    out_on, out_off = on(x), off(x)
    torch.testing.assert_close(out_on, out_off, rtol=1e-6, atol=1e-6)
    on.loss(out_on, y).backward()
    off.loss(out_off, y).backward()
    for (name, p_on), (_, p_off) in zip(on.named_parameters(),
                                        off.named_parameters()):
        assert (p_on.grad is None) == (p_off.grad is None), name
        if p_on.grad is not None:
            torch.testing.assert_close(p_on.grad, p_off.grad, rtol=1e-5, atol=1e-7,
                                       msg=lambda m, n=name: f"{n}: {m}")


def test_flag_in_config_and_checkpoints():
    from deeprest_amd.engine.config import EngineConfig, apply_cli_overrides

    spec = _tiny_spec()
    assert DeepRestNetConfig().fused_head_grad is True
    model = DeepRestNet(spec, _tiny_cfg(False))
    state = model.full_state()
    assert state["config"]["fused_head_grad"] is False
    assert DeepRestNet.from_full_state(state).cfg.fused_head_grad is False
    state["config"]["fused_head_grad"] = True
    assert DeepRestNet.from_full_state(state).cfg.fused_head_grad is True
    # a checkpoint from before the flag existed loads through the default
    del state["config"]["fused_head_grad"]
    loaded = DeepRestNet.from_full_state(state)
    assert loaded.cfg.fused_head_grad is True
    assert list(loaded.state_dict().keys()) == list(model.state_dict().keys())
    cfg = apply_cli_overrides(EngineConfig(), ["model.fused_head_grad=false"])
    assert cfg.model.fused_head_grad is False
