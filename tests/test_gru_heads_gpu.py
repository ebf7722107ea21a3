"""GPU tests of ops.fused_gru_heads: the GRU sequence kernel whose backward
takes the quantile heads' O-wide output gradient and forms the head input
gradient itself (gru_bwd_kernel<*, *, FUSED>).

Every case is compared with the fp32 composition reference_gru_sequence +
F.linear: output and the gradients of x_gates, w_hh, b_hh, h0, gamma, beta and
w_head, in both time directions.  Tolerances are the GRU tiers of
test_ops_gpu.py: forward rtol 5e-2 / atol 3e-2; gradients rtol 8e-2 / atol
5e-2 on small shapes and max error / max magnitude < 2e-2 on the large-row
shapes (their sums run over ~10^4..10^5 bf16 products, so absolute bounds do
not apply).
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

H = 128
NAMES = ["x_gates", "w_hh", "b_hh", "h0", "gamma", "beta", "w_head"]

# (B, T, C, O) — each the smallest shape that reaches its branch
SMALL = [
    (3, 7, 5, 9),      # 4-wave kernel (NSUB=1), baseline
    (2, 1, 3, 9),      # T=1: the h0 boundary is the only step
    (5, 4, 13, 9),     # R=65: ragged last 64-row tile
    (3, 5, 4, 1),      # O=1
    (3, 5, 4, 8),      # exactly one lane group of the A-fragment
    (3, 5, 4, 16),     # exactly two
    (3, 5, 4, 17),     # one element into the third
    (3, 5, 4, 32),     # full K=32
]
LARGE = [
    (400, 3, 64, 9),   # 200 128-row tiles: 8-wave LDS kernel (NSUB=2)
    (3080, 2, 8, 15),  # NSUB=2 with a ragged tail block and odd O
]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeprest_amd.ops import native_available

    if not native_available():
        pytest.fail("HIP extension not built — GPU tests must not fall back")
    return torch.device("cuda:0")


def _inputs(shape, dtype):
    B, T, C, O = shape
    gen = torch.Generator().manual_seed(1000 * B + 100 * T + 10 * C + O)
    mk = lambda *s: torch.randn(*s, generator=gen) * 0.4
    ins = [mk(B, T, 3 * H), mk(3 * H, H) / H ** 0.5, mk(3 * H) * 0.2,
           mk(B, C, H), 1.0 + 0.1 * mk(C, 3 * H), 0.1 * mk(C, 3 * H),
           mk(O, H) / H ** 0.5]
    grad = torch.randn(B, T, C, O, generator=gen)
    # b_hh stays fp32 (the op takes it as such); the rest carry the dtype
    ins = [t if i == 2 else t.to(dtype) for i, t in enumerate(ins)]
    return ins, grad.to(dtype)


def _run(fn, ins, grad, reverse):
    leaves = [t.detach().clone().requires_grad_(True) for t in ins]
    out = fn(*leaves, reverse=reverse)
    out.backward(grad)
    return out.detach().float(), [t.grad.detach().float() for t in leaves]


def _composed(xg, w_hh, b_hh, h0, gamma, beta, w_head, reverse):
    from deeprest_amd.ops import reference_gru_sequence

    return F.linear(reference_gru_sequence(xg, w_hh, b_hh, h0, gamma, beta,
                                           reverse=reverse), w_head)


def _unfused(xg, w_hh, b_hh, h0, gamma, beta, w_head, reverse):
    from deeprest_amd.ops import fused_gru_sequence

    h_all = fused_gru_sequence(xg, w_hh, b_hh, h0, gamma, beta, reverse=reverse)
    return F.linear(h_all, w_head.to(h_all.dtype))


@functools.lru_cache(maxsize=None)
def _case(shape, reverse, dtype):
    """Inputs on the device and the fp32 reference result, computed once per
    (shape, direction, dtype) and shared by the tests below."""
    dev = torch.device("cuda:0")
    ins, grad = _inputs(shape, dtype)
    ins = [t.to(dev) for t in ins]
    grad = grad.to(dev)
    ref = _run(_composed, [t.float() for t in ins], grad.float(), reverse)
    return ins, grad, ref


def _check(got, ref, large, what):
    out, grads = got
    out_r, grads_r = ref
    assert out.shape == out_r.shape
    torch.testing.assert_close(out, out_r, rtol=5e-2, atol=3e-2,
                               msg=lambda m: f"{what} output: {m}")
    for name, g, g_r in zip(NAMES, grads, grads_r):
        assert torch.isfinite(g).all(), f"{what} {name}: non-finite gradient"
        if large:
            err = (g - g_r).abs().max()
            scale = g_r.abs().max() + 1e-9
            assert err / scale < 2e-2, (
                f"{what} {name}: relmax {(err / scale).item():.4f}")
        else:
            torch.testing.assert_close(
                g, g_r, rtol=8e-2, atol=5e-2,
                msg=lambda m, n=name: f"{what} grad mismatch for {n}: {m}")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", SMALL + LARGE)
def test_matches_reference(dev, shape, reverse):
    from deeprest_amd.ops import fused_gru_heads

    ins, grad, ref = _case(shape, reverse, torch.float32)
    _check(_run(fused_gru_heads, ins, grad, reverse), ref, shape in LARGE,
           f"{shape}")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", [SMALL[0], LARGE[0]])
def test_bf16_inputs(dev, shape, reverse):
    from deeprest_amd.ops import fused_gru_heads

    ins, grad, ref = _case(shape, reverse, torch.bfloat16)
    out, grads = _run(fused_gru_heads, ins, grad, reverse)
    _check((out, grads), ref, shape in LARGE, f"bf16 {shape}")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", [SMALL[0], SMALL[6], LARGE[1]])
def test_fused_agrees_with_unfused(dev, shape, reverse):
    """Same inputs through the O-wide kernel entry and through the plain one
    fed by autograd's F.linear backward: both within the reference tiers, and
    the forward output is the same GEMM on the same h_all."""
    from deeprest_amd.ops import fused_gru_heads

    ins, grad, ref = _case(shape, reverse, torch.float32)
    fused = _run(fused_gru_heads, ins, grad, reverse)
    plain = _run(_unfused, ins, grad, reverse)
    _check(fused, ref, shape in LARGE, f"fused {shape}")
    _check(plain, ref, shape in LARGE, f"unfused {shape}")
    _check(fused, plain, shape in LARGE, f"fused vs unfused {shape}")


@pytest.mark.parametrize("shape", [(3, 5, 4, 9), (3, 5, 4, 17), (400, 2, 64, 9)])
def test_padding_never_reaches_the_result(dev, shape):
    """grad_part is the head of a larger allocation whose tail is NaN, and
    holds large finite values itself: lanes of the A-fragment past O (and past
    the last row) must contribute exact zeros, so the gradients stay finite
    and equal to the unfused path's on the same inputs."""
    from deeprest_amd.ops import fused_gru_heads

    B, T, C, O = shape
    ins, grad = _inputs(shape, torch.float32)
    ins = [t.to(dev) for t in ins]
    n = grad.numel()
    buf = torch.full((n + 4096,), float("nan"), device=dev)
    buf[:n] = (grad * 64.0).reshape(-1).to(dev)
    big = buf[:n].view(B, T, C, O)
    assert big.is_contiguous() and big.data_ptr() == buf.data_ptr()
    fused = _run(fused_gru_heads, ins, big, False)
    plain = _run(_unfused, ins, big.clone(), False)
    for name, g, g_p in zip(NAMES, fused[1], plain[1]):
        assert torch.isfinite(g).all(), name
        err = (g - g_p).abs().max()
        scale = g_p.abs().max() + 1e-9
        assert err / scale < 2e-2, f"{name}: relmax {(err / scale).item():.4f}"


@pytest.mark.parametrize("reverse", [False, True])
def test_wide_heads_take_the_unfused_path(dev, reverse, monkeypatch):
    from deeprest_amd.ops import fused_gru_heads
    from deeprest_amd.ops import gru as gru_mod

    def boom(*a, **k):
        raise AssertionError("O=33 must not reach the fused backward entry")

    monkeypatch.setattr(gru_mod._FusedGRUHeads, "apply", boom)
    shape = (3, 5, 4, 33)
    ins, grad, ref = _case(shape, reverse, torch.float32)
    _check(_run(fused_gru_heads, ins, grad, reverse), ref, False, f"{shape}")


def test_binding_rejects_bad_widths(dev):
    """The kernel entry itself refuses an O it cannot hold and a weight image
    of the wrong shape (it would index outside the (H, 32) image)."""
    from deeprest_amd.ops import gru as gru_mod
    from deeprest_amd.ops.native import require_native

    ext = require_native("test")
    B, T, C = 2, 2, 3
    ins, _ = _inputs((B, T, C, 9), torch.float32)
    xg, w_hh, b_hh, h0, gamma, beta, _ = [t.to(dev) for t in ins]
    h_all, saves = ext.gru_seq_forward(xg, w_hh, b_hh, h0, gamma, beta, False, True)
    w_img, w_fwd = gru_mod._bwd_weight_images(w_hh)
    img = torch.zeros(H, 32, device=dev, dtype=torch.bfloat16)
    args = (w_img, w_fwd, xg, gamma, beta, b_hh, h0, h_all, saves, False)
    with pytest.raises(RuntimeError):
        ext.gru_seq_backward_heads_kernel(
            torch.zeros(B, T, C, 33, device=dev), img, *args)
    with pytest.raises(RuntimeError):
        ext.gru_seq_backward_heads_kernel(
            torch.zeros(B, T, C, 9, device=dev), img[:, :16].contiguous(), *args)
    with pytest.raises(RuntimeError):
        ext.gru_seq_backward_heads_kernel(
            torch.zeros(B, T + 1, C, 9, device=dev), img, *args)


# -------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def model_setup(dev):
    from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
    from deeprest_amd.models.net import build_model_spec

    app = SyntheticApp(SyntheticAppConfig(
        n_apis=8, n_components=8, windows_per_day=120, n_days=1, seed=11))
    spec = build_model_spec(app.generate_featurized())
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(4, 30, spec.num_paths, generator=gen).to(dev)
    y = torch.rand(4, 30, spec.num_metrics, generator=gen).to(dev)
    return spec, x, y


def _cfg(fused, dropout):
    from deeprest_amd.models.net import DeepRestNetConfig

    return DeepRestNetConfig(d_model=64, n_heads=2, n_layers=1, d_ff=128,
                             hidden=128, comp_dim=16, dropout=dropout,
                             fused_head_grad=fused)


@pytest.fixture
def op_calls(monkeypatch):
    """Counts calls of the fused op as the model sees it."""
    from deeprest_amd.models import net

    calls = []
    real = net.fused_gru_heads

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(net, "fused_gru_heads", counted)
    return calls


def _step(model, x, y):
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        loss = model.loss(model(x).float(), y)
    loss.backward()
    return loss


def test_model_routing(dev, model_setup, op_calls):
    from deeprest_amd.models.net import DeepRestNet

    spec, x, y = model_setup
    torch.manual_seed(3)
    # active head dropout: today's dropout + bigk_linear path
    model = DeepRestNet(spec, _cfg(True, 0.1)).to(dev).train()
    assert torch.isfinite(_step(model, x, y))
    assert len(op_calls) == 0
    # the same model in eval mode, and a dropout-free one in training: fused,
    # once per direction
    model.eval()
    with torch.no_grad():
        model(x)
    assert len(op_calls) == 2
    del op_calls[:]
    model = DeepRestNet(spec, _cfg(True, 0.0)).to(dev).train()
    assert torch.isfinite(_step(model, x, y))
    assert len(op_calls) == 2
    del op_calls[:]
    model = DeepRestNet(spec, _cfg(False, 0.0)).to(dev).train()
    assert torch.isfinite(_step(model, x, y))
    assert len(op_calls) == 0


def test_model_flag_on_matches_off(dev, model_setup):
    """One bf16 training step, flag on vs off, same weights: the forward is
    the same kernels and GEMMs (bit-identical loss), the gradients differ only
    in that the head term is no longer rounded to bf16 before it is added."""
    from deeprest_amd.models.net import DeepRestNet

    spec, x, y = model_setup
    torch.manual_seed(3)
    off = DeepRestNet(spec, _cfg(False, 0.0)).to(dev).train()
    on = DeepRestNet(spec, _cfg(True, 0.0)).to(dev).train()
    on.load_state_dict(off.state_dict())
    loss_on, loss_off = _step(on, x, y), _step(off, x, y)
    assert torch.equal(loss_on, loss_off)
    for (name, p_on), (_, p_off) in zip(on.named_parameters(),
                                        off.named_parameters()):
        assert (p_on.grad is None) == (p_off.grad is None), name
        if p_on.grad is None:
            continue
        err = (p_on.grad - p_off.grad).abs().max()
        scale = p_off.grad.abs().max() + 1e-9
        assert err / scale < 2e-2, f"{name}: relmax {(err / scale).item():.4f}"


def test_graphed_train_step_captures_fused_heads(dev, model_setup, op_calls):
    from deeprest_amd.engine.graphstep import GraphedTrainStep
    from deeprest_amd.models.net import DeepRestNet
    from deeprest_amd.ops.adam import FusedAdam

    spec, x, y = model_setup
    torch.manual_seed(3)
    model = DeepRestNet(spec, _cfg(True, 0.0)).to(dev)
    opt = FusedAdam(model.parameters(), lr=1e-3, capturable=True)
    g = GraphedTrainStep.build(model, opt, lambda o, t: model.loss(o.float(), t),
                               x, y, autocast_dtype=torch.bfloat16, warmup=2)
    assert g is not None, "capture failed"
    assert len(op_calls) >= 2
    losses = torch.stack([g.run(x, y).detach().clone() for _ in range(6)])
    assert torch.isfinite(losses).all()
    assert losses[-1] < losses[0]
