"""CPU tests of the inference decode op (ops.fused_gru_decode) and of the
model flag that routes eval-time decoding through it (cfg.fused_head_decode).

Off the native kernel the op is reference_gru_sequence followed by F.linear
and a boundary slice, and the model does not take the decode route at all, so
everything here is exact."""

import pytest
import torch
import torch.nn.functional as F

from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig, build_model_spec
from deeprest_amd.ops import fused_gru_decode, reference_gru_sequence


def _op_inputs(B, T, C, H, O, seed=0):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=gen) * 0.4
    return [mk(B, T, 3 * H), mk(3 * H, H) / H ** 0.5, mk(3 * H) * 0.2,
            mk(B, C, H), 1.0 + 0.1 * mk(C, 3 * H), 0.1 * mk(C, 3 * H),
            mk(O, H) / H ** 0.5]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 4, 128, 9), (3, 4, 2, 16, 6),
                                   (2, 3, 3, 128, 33)])
def test_reference_path_is_gru_then_linear_and_boundary(shape, reverse):
    B, T, C, H, O = shape
    ins = _op_inputs(B, T, C, H, O)
    out, h_last = fused_gru_decode(*ins, reverse=reverse)
    h_all = reference_gru_sequence(*ins[:6], reverse=reverse)
    assert out.shape == (B, T, C, O) and h_last.shape == (B, C, H)
    assert torch.equal(out, F.linear(h_all, ins[6]))
    assert torch.equal(h_last, h_all[:, 0 if reverse else -1])


@pytest.mark.parametrize("which", [0, 3, 6])
def test_raises_when_grad_is_required(which):
    ins = _op_inputs(2, 3, 4, 128, 9)
    ins[which].requires_grad_(True)
    with pytest.raises(RuntimeError):
        fused_gru_decode(*ins)
    with torch.no_grad():                      # fine once grad mode is off
        out, _ = fused_gru_decode(*ins)
    assert not out.requires_grad


# -------------------------------------------------------------------- model
def _tiny_spec():
    app = SyntheticApp(SyntheticAppConfig(
        n_apis=3, n_components=4, windows_per_day=30, n_days=2, seed=3))
    return build_model_spec(app.generate_featurized())


def _tiny_cfg(decode):
    return DeepRestNetConfig(d_model=32, n_heads=4, n_layers=1, d_ff=64,
                             hidden=16, comp_dim=8, dropout=0.0,
                             fused_head_decode=decode)


def test_cpu_model_flag_changes_nothing():
    spec = _tiny_spec()
    torch.manual_seed(0)
    off = DeepRestNet(spec, _tiny_cfg(False)).eval()
    on = DeepRestNet(spec, _tiny_cfg(True)).eval()
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    on.load_state_dict(off.state_dict())
    x = torch.randn(2, 12, spec.num_paths,
                    generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        assert torch.equal(on(x), off(x))
        assert torch.equal(on.forward_long(x, chunk_size=5),
                           off.forward_long(x, chunk_size=5))


def test_flag_in_config_and_checkpoints():
    from deeprest_amd.engine.config import EngineConfig, apply_cli_overrides

    spec = _tiny_spec()
    assert DeepRestNetConfig().fused_head_decode is False
    model = DeepRestNet(spec, _tiny_cfg(True))
    state = model.full_state()
    assert state["config"]["fused_head_decode"] is True
    assert DeepRestNet.from_full_state(state).cfg.fused_head_decode is True
    # a checkpoint from before the flag existed loads through the default
    del state["config"]["fused_head_decode"]
    loaded = DeepRestNet.from_full_state(state)
    assert loaded.cfg.fused_head_decode is False
    assert list(loaded.state_dict().keys()) == list(model.state_dict().keys())
    cfg = apply_cli_overrides(EngineConfig(), ["model.fused_head_decode=true"])
    assert cfg.model.fused_head_decode is True
