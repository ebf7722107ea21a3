"""GPU numerics tests: each HIP kernel vs the plain PyTorch fp32 reference.

Tolerance tiers: bf16 internal compute (GRU/MHA GEMM operands, guide section 4)
is compared against the fp32 oracle at bf16-appropriate tolerances; fp32-only
kernels (pinball, adam, layernorm stats) at fp32 tolerances.
"""

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeprest_amd.ops import native_available

    if not native_available():
        pytest.fail("HIP extension not built — GPU tests must not fall back")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ layernorm
# strided tier below 256 with D % 4 != 0; streaming tier; one past 64 values
# per lane; grid-stride loop past 2048 blocks x 4 waves.  These get the
# upstream gradient rounded to the IO dtype for kernel AND reference: over
# 8200 bf16 rows the rounding of g itself adds ~sqrt(8200) * 2^-9 = 0.18 per
# unit of gradient to dw, which is the test's error and not the kernel's.
_LN_ROUNDED_G_SHAPES = [(3, 70), (3, 1090), (2, 4100), (8200, 64)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(8, 16, 256), (3, 7, 192), (1, 1, 64), (5, 1024)]
                         + _LN_ROUNDED_G_SHAPES)
def test_layernorm_fwd_bwd(dev, dtype, shape):
    from deeprest_amd.ops import layer_norm, reference_layer_norm

    torch.manual_seed(0)
    x = torch.randn(*shape, device=dev, dtype=dtype) * 3 + 1
    w = torch.randn(shape[-1], device=dev) * 0.5 + 1.0
    b = torch.randn(shape[-1], device=dev) * 0.1
    x_ref = x.detach().float().requires_grad_(True)
    w_ref = w.detach().clone().requires_grad_(True)
    b_ref = b.detach().clone().requires_grad_(True)
    x_t = x.detach().clone().requires_grad_(True)
    w_t = w.detach().clone().requires_grad_(True)
    b_t = b.detach().clone().requires_grad_(True)

    y = layer_norm(x_t, w_t, b_t)
    y_ref = reference_layer_norm(x_ref, w_ref, b_ref)
    tol = dict(rtol=2e-2, atol=2e-2) if dtype == torch.bfloat16 else dict(rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(y.float(), y_ref, **tol)

    g = torch.randn_like(y_ref)
    if shape in _LN_ROUNDED_G_SHAPES:
        g = g.to(dtype).float()
    y.backward(g.to(dtype))
    y_ref.backward(g)
    torch.testing.assert_close(x_t.grad.float(), x_ref.grad, rtol=5e-2 if dtype == torch.bfloat16 else 1e-4,
                               atol=5e-2 if dtype == torch.bfloat16 else 1e-4)
    torch.testing.assert_close(w_t.grad, w_ref.grad, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(b_t.grad, b_ref.grad, rtol=5e-2, atol=5e-2)


def test_layernorm_backward_rejects_wide_rows(dev):
    """dw/db partials take 2 * D floats of LDS per block: D > 8192 must raise
    before any launch, not return an unwritten dx."""
    from deeprest_amd.ops import layer_norm

    D = 8200
    x = torch.randn(1, D, device=dev, requires_grad=True)
    w = torch.ones(D, device=dev, requires_grad=True)
    b = torch.zeros(D, device=dev, requires_grad=True)
    y = layer_norm(x, w, b)
    torch.testing.assert_close(y, torch.nn.functional.layer_norm(x, (D,), w, b),
                               rtol=2e-5, atol=2e-5)
    with pytest.raises(RuntimeError, match="8192"):
        y.sum().backward()
    assert x.grad is None and w.grad is None and b.grad is None


# -------------------------------------------------------------------- pinball
def test_pinball_fwd_bwd(dev):
    from deeprest_amd.ops import pinball_loss, reference_pinball_loss

    torch.manual_seed(1)
    B, T, M, Q = 4, 12, 9, 3
    quantiles = (0.05, 0.50, 0.95)
    out = torch.randn(B, T, M, Q, device=dev)
    lab = torch.randn(B, T, M, device=dev)
    out_t = out.detach().clone().requires_grad_(True)
    out_r = out.detach().clone().requires_grad_(True)

    l_t = pinball_loss(out_t, lab, quantiles)
    l_r = reference_pinball_loss(out_r, lab, quantiles)
    torch.testing.assert_close(l_t, l_r, rtol=1e-5, atol=1e-6)
    l_t.backward()
    l_r.backward()
    torch.testing.assert_close(out_t.grad, out_r.grad, rtol=1e-5, atol=1e-7)


# ----------------------------------------------------------------- fused adam
def test_fused_adam_matches_torch(dev):
    from deeprest_amd.ops.adam import FusedAdam

    torch.manual_seed(2)
    shapes = [(64, 32), (128,), (7, 5, 3), (1000,)]
    params_a = [torch.randn(*s, device=dev, requires_grad=True) for s in shapes]
    params_b = [p.detach().clone().requires_grad_(True) for p in params_a]
    opt_a = FusedAdam(params_a, lr=1e-2, weight_decay=0.01)
    opt_b = torch.optim.Adam(params_b, lr=1e-2, weight_decay=0.01)
    for step in range(5):
        for pa, pb in zip(params_a, params_b):
            g = torch.randn_like(pa)
            pa.grad = g.clone()
            pb.grad = g.clone()
        opt_a.step()
        opt_b.step()
    for pa, pb in zip(params_a, params_b):
        torch.testing.assert_close(pa, pb, rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------ gru
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("reverse", [False, True])
def test_gru_forward_matches_reference(dev, dtype, reverse):
    from deeprest_amd.ops import fused_gru_sequence, reference_gru_sequence

    torch.manual_seed(3)
    B, T, C, H = 3, 7, 5, 128
    xg = torch.randn(B, T, 3 * H, device=dev, dtype=dtype) * 0.5
    w_hh = (torch.randn(3 * H, H, device=dev) * (1.0 / np.sqrt(H))).to(dtype)
    b_hh = torch.randn(3 * H, device=dev) * 0.1
    h0 = torch.randn(B, C, H, device=dev, dtype=dtype) * 0.3
    gamma = (1.0 + 0.1 * torch.randn(C, 3 * H, device=dev)).to(dtype)
    beta = (0.1 * torch.randn(C, 3 * H, device=dev)).to(dtype)

    out = fused_gru_sequence(xg, w_hh, b_hh, h0, gamma, beta, reverse=reverse)
    ref = reference_gru_sequence(
        xg.float(), w_hh.float(), b_hh.float(), h0.float(),
        gamma.float(), beta.float(), reverse=reverse,
    )
    assert out.shape == (B, T, C, H)
    torch.testing.assert_close(out.float(), ref, rtol=5e-2, atol=3e-2)


def test_gru_forward_large_rows_tail(dev):
    # R not a multiple of 64 exercises the pad-row path
    from deeprest_amd.ops import fused_gru_sequence, reference_gru_sequence

    torch.manual_seed(4)
    B, T, C, H = 5, 4, 13, 128  # R = 65
    xg = torch.randn(B, T, 3 * H, device=dev) * 0.5
    w_hh = torch.randn(3 * H, H, device=dev) / np.sqrt(H)
    b_hh = torch.zeros(3 * H, device=dev)
    h0 = torch.zeros(B, C, H, device=dev)
    out = fused_gru_sequence(xg, w_hh, b_hh, h0)
    ref = reference_gru_sequence(xg, w_hh, b_hh, h0)
    torch.testing.assert_close(out.float(), ref, rtol=5e-2, atol=3e-2)
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("reverse", [False, True])
def test_gru_backward_matches_reference(dev, reverse):
    from deeprest_amd.ops import fused_gru_sequence, reference_gru_sequence

    torch.manual_seed(5)
    B, T, C, H = 2, 5, 4, 128
    mk = lambda *s: torch.randn(*s, device=dev) * 0.4

    xg0, w0, b0, h00 = mk(B, T, 3 * H), mk(3 * H, H) / np.sqrt(H), mk(3 * H) * 0.2, mk(B, C, H)
    g0 = 1.0 + 0.1 * mk(C, 3 * H)
    be0 = 0.1 * mk(C, 3 * H)

    args_t = [t.detach().clone().requires_grad_(True) for t in (xg0, w0, b0, h00, g0, be0)]
    args_r = [t.detach().clone().requires_grad_(True) for t in (xg0, w0, b0, h00, g0, be0)]

    out_t = fused_gru_sequence(*args_t, reverse=reverse)
    out_r = reference_gru_sequence(*args_r, reverse=reverse)
    grad = torch.randn_like(out_r)
    out_t.backward(grad)
    out_r.backward(grad)

    names = ["x_gates", "w_hh", "b_hh", "h0", "gamma", "beta"]
    for name, at_, ar_ in zip(names, args_t, args_r):
        assert at_.grad is not None, name
        torch.testing.assert_close(
            at_.grad.float(), ar_.grad.float(), rtol=8e-2, atol=5e-2,
            msg=lambda m, n=name: f"grad mismatch for {n}: {m}",
        )


# ------------------------------------------------------------------------ mha
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T_len", [60, 64, 37, 128])
@pytest.mark.parametrize("D", [32, 64, 16])
def test_mha_forward_matches_reference(dev, dtype, T_len, D):
    from deeprest_amd.ops import mha_forward, reference_mha

    torch.manual_seed(6)
    B, NH = 2, 4
    q = torch.randn(B, NH, T_len, D, device=dev, dtype=dtype)
    k = torch.randn(B, NH, T_len, D, device=dev, dtype=dtype)
    v = torch.randn(B, NH, T_len, D, device=dev, dtype=dtype)
    o = mha_forward(q, k, v)
    o_ref = reference_mha(q.float(), k.float(), v.float())
    torch.testing.assert_close(o.float(), o_ref, rtol=3e-2, atol=2e-2)


def test_mha_asymmetric_catches_transpose(dev):
    # asymmetric K/V catch row<->col swaps (guide: always test with asymmetric B)
    from deeprest_amd.ops import mha_forward, reference_mha

    B, NH, T_len, D = 1, 1, 32, 32
    q = torch.zeros(B, NH, T_len, D, device=dev)
    q[0, 0, :, 0] = torch.arange(T_len, device=dev) * 0.1
    k = torch.zeros_like(q)
    k[0, 0, :, 0] = torch.arange(T_len, device=dev) * 0.05
    v = torch.arange(T_len * D, device=dev, dtype=torch.float32).reshape(1, 1, T_len, D) * 0.01
    o = mha_forward(q, k, v)
    o_ref = reference_mha(q, k, v)
    torch.testing.assert_close(o.float(), o_ref, rtol=2e-2, atol=2e-2)


def test_mha_backward_matches_reference(dev):
    from deeprest_amd.ops import mha_forward, reference_mha

    torch.manual_seed(7)
    B, NH, T_len, D = 2, 3, 60, 32
    mk = lambda: torch.randn(B, NH, T_len, D, device=dev) * 0.7
    q0, k0, v0 = mk(), mk(), mk()
    qt, kt, vt = (t.detach().clone().requires_grad_(True) for t in (q0, k0, v0))
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q0, k0, v0))
    o_t = mha_forward(qt, kt, vt)
    o_r = reference_mha(qr, kr, vr)
    g = torch.randn_like(o_r)
    o_t.backward(g)
    o_r.backward(g)
    for a, b in ((qt, qr), (kt, kr), (vt, vr)):
        torch.testing.assert_close(a.grad, b.grad, rtol=5e-2, atol=3e-2)


# -------------------------------------------------------------- model-on-gpu
def test_model_step_on_gpu(dev):
    from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
    from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig, build_model_spec
    from deeprest_amd.ops.adam import FusedAdam

    app = SyntheticApp(SyntheticAppConfig(
        n_apis=8, n_components=8, windows_per_day=120, n_days=1, seed=11))
    data = app.generate_featurized()
    spec = build_model_spec(data)
    model = DeepRestNet(spec, DeepRestNetConfig(
        d_model=64, n_heads=2, n_layers=1, d_ff=128, hidden=128, comp_dim=16,
        dropout=0.0)).to(dev)
    opt = FusedAdam(model.parameters(), lr=1e-3)
    x = torch.randn(4, 30, spec.num_paths, device=dev)
    y = torch.rand(4, 30, spec.num_metrics, device=dev)
    losses = []
    for _ in range(10):
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            out = model(x)
            loss = model.loss(out.float(), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0]


def test_graphed_train_step(dev):
    """Whole-step hipGraph capture: loss keeps decreasing across replays and
    stays consistent with an identically-seeded eager run."""
    from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
    from deeprest_amd.engine.graphstep import GraphedTrainStep
    from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig, build_model_spec
    from deeprest_amd.ops.adam import FusedAdam

    app = SyntheticApp(SyntheticAppConfig(
        n_apis=8, n_components=8, windows_per_day=120, n_days=1, seed=11))
    data = app.generate_featurized()
    spec = build_model_spec(data)
    cfg = DeepRestNetConfig(d_model=64, n_heads=2, n_layers=1, d_ff=128,
                            hidden=128, comp_dim=16, dropout=0.0)
    x = torch.randn(4, 30, spec.num_paths, device=dev)
    y = torch.rand(4, 30, spec.num_metrics, device=dev)

    def run(graphed: bool, steps=12):
        torch.manual_seed(3)
        model = DeepRestNet(spec, cfg).to(dev)
        opt = FusedAdam(model.parameters(), lr=1e-3, capturable=graphed)
        losses = []
        g = None
        if graphed:
            g = GraphedTrainStep.build(
                model, opt, lambda o, t: model.loss(o.float(), t), x, y,
                autocast_dtype=torch.bfloat16, warmup=2)
            assert g is not None, "capture failed"
        for _ in range(steps):
            if g is not None:
                loss = g.run(x, y)
            else:
                with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                    out = model(x)
                    loss = model.loss(out.float(), y)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
            losses.append(float(loss.detach().cpu()))
        return losses

    eager = run(False)
    graphed = run(True)
    assert all(np.isfinite(graphed))
    assert graphed[-1] < graphed[0]
    # the graphed run includes its capture-warmup steps, so it is a few
    # optimizer steps ahead; both runs must land in the same converged band
    assert abs(graphed[-1] - eager[-1]) < 0.25 * abs(eager[0] - eager[-1]) + 1e-3


def test_trainer_graph_step_gpu(dev):
    """Trainer with graph_step=True captures and keeps training correctly."""
    import numpy as np

    from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
    from deeprest_amd.engine.config import EngineConfig
    from deeprest_amd.engine.trainer import Trainer
    from deeprest_amd.models.net import DeepRestNetConfig

    app = SyntheticApp(SyntheticAppConfig(
        n_apis=6, n_components=6, windows_per_day=160, n_days=1, seed=3))
    data = app.generate_featurized()
    cfg = EngineConfig()
    cfg.train.epochs = 2
    cfg.train.batch_size = 16
    cfg.train.graph_step = True
    cfg.train.run_baselines = False
    cfg.train.log_every = 0
    cfg.model = DeepRestNetConfig(d_model=64, n_heads=2, n_layers=1, d_ff=128,
                                  hidden=128, comp_dim=16, dropout=0.0)
    tr = Trainer(data, cfg, device=dev)
    res = tr.train()
    assert tr.step.graphed, "graph was not captured"
    assert np.isfinite(res.train_losses).all()
    assert res.train_losses[-1] < res.train_losses[0] * 1.5


# --------------------------------------------------------------- predictor
def test_predictor_hipgraph_capture(dev):
    import numpy as np

    from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
    from deeprest_amd.data.windows import MinMaxScaler, sliding_window
    from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig, build_model_spec
    from deeprest_amd.serve.predictor import Predictor

    app = SyntheticApp(SyntheticAppConfig(
        n_apis=6, n_components=6, windows_per_day=150, n_days=1, seed=17))
    data = app.generate_featurized()
    spec = build_model_spec(data)
    model = DeepRestNet(spec, DeepRestNetConfig(
        d_model=64, n_heads=2, n_layers=1, d_ff=128, hidden=128, comp_dim=16,
        dropout=0.0)).to(dev).eval()

    x_scaler = MinMaxScaler().fit(data.traffic.astype(np.float64), 100)
    y_scalers = [MinMaxScaler() for _ in data.metric_names]
    pred_graph = Predictor(model, x_scaler, y_scalers, data.metric_names,
                           device=dev, graph_batches=(16, 64), use_graph=True)
    pred_eager = Predictor(model, x_scaler, y_scalers, data.metric_names,
                           device=dev, use_graph=False)
    w_all = sliding_window(data.traffic.astype(np.float64), 30)
    # small request -> padded replay of the 16-graph; mid request -> the
    # 64-graph; oversized request -> chunked replays of the largest graph
    for n in (12, 40, 100):
        w = np.concatenate([w_all] * (n // len(w_all) + 1))[:n]
        out_g = pred_graph.predict(w)
        out_e = pred_eager.predict(w)
        for name in data.metric_names:
            np.testing.assert_allclose(out_g[name], out_e[name],
                                       rtol=1e-3, atol=1e-3)
    assert pred_graph.captured_batches == [16, 64], "graphs not captured"
    # staged ingestion: write into the buffer, replay, same numbers
    xn = pred_graph.x_scaler.transform(w_all[:10].astype(np.float64))
    buf = pred_graph.staging_buffer(10, 30, xn.shape[-1])
    buf.copy_(torch.from_numpy(xn).float())
    out_s = pred_graph.predict_staged(10, 30)
    out_d = pred_graph.predict_normalized(
        torch.from_numpy(xn).float())
    torch.testing.assert_close(out_s, out_d, rtol=1e-5, atol=1e-5)


def test_gru_large_rows_8wave_variant(dev):
    # R = B*C >= 192*128 exercises the 8-wave LDS-W backward variant that
    # small shapes never reach
    from deeprest_amd.ops import fused_gru_sequence, reference_gru_sequence

    torch.manual_seed(8)
    B, T, C, H = 400, 3, 64, 128  # R = 25600 -> 200 x 128-row tiles
    xg = torch.randn(B, T, 3 * H, device=dev) * 0.4
    w_hh = torch.randn(3 * H, H, device=dev) / np.sqrt(H)
    b_hh = torch.randn(3 * H, device=dev) * 0.1
    h0 = torch.randn(B, C, H, device=dev) * 0.3
    gamma = 1.0 + 0.1 * torch.randn(C, 3 * H, device=dev)
    beta = 0.1 * torch.randn(C, 3 * H, device=dev)
    args_t = [t.detach().clone().requires_grad_(True)
              for t in (xg, w_hh, b_hh, h0, gamma, beta)]
    args_r = [t.detach().clone().requires_grad_(True)
              for t in (xg, w_hh, b_hh, h0, gamma, beta)]
    out_t = fused_gru_sequence(*args_t)
    out_r = reference_gru_sequence(*args_r)
    torch.testing.assert_close(out_t.float(), out_r, rtol=5e-2, atol=3e-2)
    g = torch.randn_like(out_r)
    out_t.backward(g)
    out_r.backward(g)
    # gradients here sum ~76k bf16 products: compare error relative to the
    # tensor's own scale (absolute tolerances don't scale with K)
    for name, at_, ar_ in zip(["xg", "w", "b", "h0", "gam", "bet"], args_t, args_r):
        err = (at_.grad.float() - ar_.grad.float()).abs().max()
        scale = ar_.grad.float().abs().max() + 1e-9
        assert err / scale < 2e-2, f"{name}: relmax {(err / scale).item():.4f}"


def test_gru_fp8_inference_path(dev):
    # fp8 MFMA forward (config 5): looser tolerance vs the fp32 oracle —
    # e4m3 GEMM operands with fp32 state
    from deeprest_amd.ops import fused_gru_sequence, reference_gru_sequence

    torch.manual_seed(10)
    B, T, C, H = 3, 12, 6, 128
    xg = torch.randn(B, T, 3 * H, device=dev) * 0.4
    w_hh = torch.randn(3 * H, H, device=dev) / np.sqrt(H)
    b_hh = torch.randn(3 * H, device=dev) * 0.1
    h0 = torch.randn(B, C, H, device=dev) * 0.3
    with torch.no_grad():
        out8 = fused_gru_sequence(xg, w_hh, b_hh, h0, fp8=True)
        ref = reference_gru_sequence(xg, w_hh, b_hh, h0)
    assert torch.isfinite(out8).all()
    err = (out8.float() - ref).abs().max().item()
    assert err < 0.25, f"fp8 GRU drifted too far from fp32 oracle: {err}"
    # and it must be meaningfully closer than noise: correlation check
    flat8 = out8.float().flatten()
    flatr = ref.flatten()
    corr = torch.corrcoef(torch.stack([flat8, flatr]))[0, 1].item()
    assert corr > 0.99, corr


# ------------------------------------------------------- gru edge coverage
@pytest.mark.parametrize("shape", [
    (1, 1, 3, 128),     # absolute minimum: B=1, T=1, C=3
    (1, 9, 3, 128),     # B=1
    (6, 1, 7, 128),     # T=1
    (64, 2, 3, 128),    # C=3 (launcher's minimum C) with a multi-tile grid
])
@pytest.mark.parametrize("reverse", [False, True])
def test_gru_edge_shapes_fwd_bwd(dev, shape, reverse):
    """Every edge the launcher branches on (csrc/gru.hip launchers): T=1,
    B=1, C=3 — forward AND backward vs the fp32 oracle."""
    from deeprest_amd.ops import fused_gru_sequence, reference_gru_sequence

    B, T, C, H = shape
    torch.manual_seed(11)
    mk = lambda *s: torch.randn(*s, device=dev) * 0.4
    xg, w, b, h0 = mk(B, T, 3 * H), mk(3 * H, H) / np.sqrt(H), mk(3 * H) * 0.2, mk(B, C, H)
    g, be = 1.0 + 0.1 * mk(C, 3 * H), 0.1 * mk(C, 3 * H)
    args_t = [t.detach().clone().requires_grad_(True) for t in (xg, w, b, h0, g, be)]
    args_r = [t.detach().clone().requires_grad_(True) for t in (xg, w, b, h0, g, be)]
    out_t = fused_gru_sequence(*args_t, reverse=reverse)
    out_r = reference_gru_sequence(*args_r, reverse=reverse)
    torch.testing.assert_close(out_t.float(), out_r, rtol=5e-2, atol=3e-2)
    grad = torch.randn_like(out_r)
    out_t.backward(grad)
    out_r.backward(grad)
    for name, at_, ar_ in zip(["xg", "w", "b", "h0", "gam", "bet"], args_t, args_r):
        torch.testing.assert_close(
            at_.grad.float(), ar_.grad.float(), rtol=8e-2, atol=5e-2,
            msg=lambda m, n=name: f"{shape} grad mismatch for {n}: {m}")


@pytest.mark.parametrize("B,C", [
    (3056, 8),   # 191 x 128-row tiles: NSUB1 side of the boundary
    (3072, 8),   # exactly 192 tiles: first NSUB2 launch
    (3080, 8),   # 192+ tiles with a ragged tail row block
    (6200, 4),   # big grid but C=4: fwd stays NSUB1 (C>=5 gate)
])
def test_gru_nsub_boundary(dev, B, C):
    """The NSUB1/NSUB2 launcher boundary (tiles128 >= 192, fwd also C >= 5)
    — both sides must agree with the oracle, fwd and bwd."""
    from deeprest_amd.ops import fused_gru_sequence, reference_gru_sequence

    T, H = 2, 128
    torch.manual_seed(12)
    mk = lambda *s: torch.randn(*s, device=dev) * 0.4
    xg, w, b, h0 = mk(B, T, 3 * H), mk(3 * H, H) / np.sqrt(H), mk(3 * H) * 0.2, mk(B, C, H)
    g, be = 1.0 + 0.1 * mk(C, 3 * H), 0.1 * mk(C, 3 * H)
    args_t = [t.detach().clone().requires_grad_(True) for t in (xg, w, b, h0, g, be)]
    args_r = [t.detach().clone().requires_grad_(True) for t in (xg, w, b, h0, g, be)]
    out_t = fused_gru_sequence(*args_t)
    out_r = reference_gru_sequence(*args_r)
    torch.testing.assert_close(out_t.float(), out_r, rtol=5e-2, atol=3e-2)
    grad = torch.randn_like(out_r)
    out_t.backward(grad)
    out_r.backward(grad)
    for name, at_, ar_ in zip(["xg", "w", "b", "h0", "gam", "bet"], args_t, args_r):
        err = (at_.grad.float() - ar_.grad.float()).abs().max()
        scale = ar_.grad.float().abs().max() + 1e-9
        assert err / scale < 2e-2, f"{name}: relmax {(err / scale).item():.4f}"


def test_gru_offspec_shape_uses_composed_path(dev):
    """hidden != 128 / C < 3 degrade to the differentiable rocBLAS
    composition with a one-time warning — defined behavior, not a crash
    and not a silent wrong answer."""
    import warnings

    from deeprest_amd.ops import fused_gru_sequence, reference_gru_sequence
    from deeprest_amd.ops.gru import _WARNED_SHAPES

    torch.manual_seed(13)
    for (B, T, C, H) in [(4, 5, 6, 64), (4, 5, 2, 128)]:
        _WARNED_SHAPES.clear()
        mk = lambda *s: torch.randn(*s, device=dev) * 0.4
        xg, w, b, h0 = mk(B, T, 3 * H), mk(3 * H, H) / np.sqrt(H), mk(3 * H) * 0.2, mk(B, C, H)
        args = [t.detach().clone().requires_grad_(True) for t in (xg, w, b, h0)]
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            out = fused_gru_sequence(*args)
        assert any("composed rocBLAS path" in str(r.message) for r in rec)
        ref = reference_gru_sequence(xg, w, b, h0)
        torch.testing.assert_close(out.float(), ref.float(), rtol=1e-4, atol=1e-4)
        out.sum().backward()   # autograd must work on the degraded path
        assert args[0].grad is not None and torch.isfinite(args[0].grad).all()


def test_pinball_bf16_outputs(dev):
    """bf16 predictions feed the pinball kernel directly; loss and grads
    match the fp32 oracle at bf16 tolerance."""
    from deeprest_amd.ops import pinball_loss
    from deeprest_amd.ops.pinball import reference_pinball_loss

    torch.manual_seed(6)
    B, T, M, Q = 4, 9, 5, 3
    out16 = (torch.randn(B, T, M, Q, device=dev) * 0.5).to(torch.bfloat16)
    labels = torch.randn(B, T, M, device=dev)
    a = out16.detach().clone().requires_grad_(True)
    b = out16.float().detach().clone().requires_grad_(True)
    la = pinball_loss(a, labels)
    lb = reference_pinball_loss(b, labels, (0.05, 0.50, 0.95))
    assert la.dtype == torch.float32
    torch.testing.assert_close(la, lb.float(), rtol=2e-2, atol=1e-3)
    la.backward()
    lb.backward()
    assert a.grad.dtype == torch.bfloat16
    torch.testing.assert_close(a.grad.float(), b.grad, rtol=2e-2, atol=2e-3)


def test_resource_aware_batch_on_device(dev):
    """Batched RESRC baseline on GPU == CPU sequential at full batch."""
    from deeprest_amd.models.baselines import (ResourceAwareBaseline,
                                               ResourceAwareBatchBaseline)

    rng = np.random.default_rng(7)
    M, N, W = 4, 80, 12
    y = np.cumsum(rng.normal(1.0, 0.3, size=(M, N, W)), axis=1) + 5.0
    gpu_out = ResourceAwareBatchBaseline(
        split=40, window=W, epochs=3, batch_size=10**6, seed=3,
        device=dev).fit_and_estimate(y)
    cpu_out = ResourceAwareBatchBaseline(
        split=40, window=W, epochs=3, batch_size=10**6, seed=3
    ).fit_and_estimate(y)
    np.testing.assert_allclose(gpu_out, cpu_out, rtol=2e-4, atol=2e-4)


def test_bench_graph_cycle_env(dev):
    """DEEPREST_GRAPH_STEP=1 runs the zero-copy multi-graph training cycle
    end-to-end (off by default; measured slower at the flagship config but
    a supported mode)."""
    import json as _json
    import os as _os
    import subprocess
    import sys as _sys

    repo = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
    env = dict(_os.environ, DEEPREST_GRAPH_STEP="1")
    out = subprocess.run(
        [_sys.executable, "bench.py", "--steps", "3", "--warmup", "1",
         "--batch", "64", "--endpoints", "8", "--components", "7",
         "--seq-len", "16", "--accuracy", "off"],
        cwd=repo, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][0]
    d = _json.loads(line)
    assert d["value"] > 0
    assert "graph cycle capture failed" not in out.stderr


def test_forward_long_gpu_matches_forward(dev):
    """Long-horizon streaming path on the NATIVE kernels: a single chunk
    covering the horizon equals the plain forward; multi-chunk runs stay
    finite and the fp8 decode variant tracks bf16."""
    from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
    from deeprest_amd.models.net import (DeepRestNet, DeepRestNetConfig,
                                         build_model_spec)

    app = SyntheticApp(SyntheticAppConfig(
        n_apis=5, n_components=6, windows_per_day=120, n_days=1, seed=23))
    data = app.generate_featurized()
    spec = build_model_spec(data)
    torch.manual_seed(4)
    model = DeepRestNet(spec, DeepRestNetConfig(
        d_model=64, n_heads=2, n_layers=1, d_ff=128, hidden=128, comp_dim=16,
        dropout=0.0)).to(dev).eval()
    x = torch.rand(2, 96, spec.num_paths, device=dev)
    with torch.no_grad():
        full = model(x)
        one_chunk = model.forward_long(x, chunk_size=96)
        multi = model.forward_long(x, chunk_size=32)
    torch.testing.assert_close(one_chunk, full, rtol=2e-4, atol=2e-4)
    assert multi.shape == full.shape and torch.isfinite(multi).all()

    model.cfg.fp8_inference = True
    with torch.no_grad():
        fp8_out = model.forward_long(x, chunk_size=96)
    err = (fp8_out - full).abs().max().item()
    assert err < 0.5, f"fp8 decode drifted: {err}"
