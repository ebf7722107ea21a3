"""GPU tests of the masked pinball kernels (NaN label = not observed) against
``reference_masked_pinball_loss`` evaluated in float64 on the CPU from the
same inputs.

Thread layout of the kernels (csrc/pinball.hip): column tiles of at most 256
metrics, the rest of the 256-thread block as row lanes.  The shapes straddle
what changes with M: one row lane vs several (M 128 | 129), one column tile
vs two (M 256 | 257), a row-lane count that is / is not a power of two
(M 1 | 3, 9), several blocks per column with several row lanes ((1, 700, 3)),
and the row-stride loop ((1, 4099, 130): 532,870 labels).

Tolerances, f32 outputs: loss rtol max(1e-5, rows_per_metric * 2^-24), atol
1e-6 (worst case of summing non-negative fp32 terms in any order; 1e-5/1e-6
is the tier of test_pinball_fwd_bwd); gradients rtol 1e-5, atol 1e-7, and
bitwise 0 at missing positions.  bf16 outputs: the tier of
test_pinball_bf16_outputs (loss 2e-2 / 1e-3, gradients 2e-2 / 2e-3).
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

QUANTILES = (0.05, 0.5, 0.95)
Q8 = (0.01, 0.05, 0.25, 0.4, 0.5, 0.75, 0.95, 0.99)

SHAPES = [
    (2, 3, 1, 1),
    (4, 12, 3, 3),
    (3, 7, 9, 8),
    (2, 5, 128, 3),
    (2, 5, 129, 3),
    (2, 5, 192, 3),
    (2, 5, 256, 3),
    (2, 5, 257, 3),
    (1, 700, 3, 2),
    (1, 4099, 130, 3),
]
BF16_SHAPES = [(4, 12, 3, 3), (2, 5, 257, 3), (1, 4099, 130, 3)]
PATTERNS = ["none", "random40", "one_metric", "all"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeprest_amd.ops import native_available

    if not native_available():
        pytest.fail("HIP extension not built — GPU tests must not fall back")
    return torch.device("cuda:0")


def _quantiles(Q):
    return {1: (0.5,), 2: (0.05, 0.95), 3: QUANTILES, 8: Q8}[Q]


def _missing(shape, pattern, seed=0):
    """(B, T, M) bool, True = missing."""
    B, T, M, _ = shape
    gen = torch.Generator().manual_seed(1000 + seed)
    miss = torch.zeros(B, T, M, dtype=torch.bool)
    if pattern in ("random40", "one_metric"):
        miss = torch.rand(B, T, M, generator=gen) < 0.4
        kept = ~miss
        if pattern == "one_metric":
            miss[:, :, M - 1] = True
            kept = kept[:, :, : M - 1]
        # nothing is emptied by accident: every other metric keeps a label
        assert kept.any(dim=0).any(dim=0).all(), "random mask emptied a metric"
        assert miss.any()
    elif pattern == "all":
        miss[:] = True
    return miss


_CASES = {}


def _case(shape, pattern, dtype=torch.float32, seed=0):
    """Inputs on the CPU plus the float64 reference loss and gradient; built
    once per (shape, pattern, dtype, seed) and never modified."""
    from deeprest_amd.ops import reference_masked_pinball_loss

    key = (shape, pattern, dtype, seed)
    if key not in _CASES:
        B, T, M, Q = shape
        gen = torch.Generator().manual_seed(7 + seed)
        out = torch.randn(B, T, M, Q, generator=gen).to(dtype)
        y = torch.rand(B, T, M, generator=gen)
        miss = _missing(shape, pattern, seed)
        y[miss] = float("nan")
        o64 = out.double().requires_grad_(True)
        loss = reference_masked_pinball_loss(o64, y.double(), _quantiles(Q))
        loss.backward()
        _CASES[key] = (out, y, miss, loss.detach(), o64.grad)
    return _CASES[key]


def _loss_tol(shape):
    B, T = shape[:2]
    return dict(rtol=max(1e-5, B * T * 2.0 ** -24), atol=1e-6)


def _run(dev, out, y, quantiles):
    from deeprest_amd.ops import masked_pinball_loss

    o = out.to(dev).requires_grad_(True)
    loss = masked_pinball_loss(o, y.to(dev), quantiles)
    loss.backward()
    return loss.detach(), o.grad


# ------------------------------------------------------------ 1. numerics
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_masked_pinball_f32(dev, shape, pattern):
    out, y, miss, ref_loss, ref_grad = _case(shape, pattern)
    loss, grad = _run(dev, out, y, _quantiles(shape[3]))
    assert loss.dtype == torch.float32 and grad.dtype == torch.float32
    print(f"{shape} {pattern}: loss {float(loss):.9g} ref {float(ref_loss):.9g} "
          f"max|dgrad| {(grad.cpu().double() - ref_grad).abs().max():.3e}")
    torch.testing.assert_close(loss.cpu().double(), ref_loss, **_loss_tol(shape))
    torch.testing.assert_close(grad.cpu().double(), ref_grad, rtol=1e-5, atol=1e-7)
    g = grad.cpu()
    assert torch.equal(g[miss], torch.zeros_like(g[miss]))      # +0.0, bitwise
    assert not torch.signbit(g[miss]).any()
    if pattern == "all":
        assert float(loss) == 0.0


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", BF16_SHAPES, ids=str)
def test_masked_pinball_bf16_outputs(dev, shape, pattern):
    out, y, miss, ref_loss, ref_grad = _case(shape, pattern, torch.bfloat16)
    loss, grad = _run(dev, out, y, _quantiles(shape[3]))
    assert loss.dtype == torch.float32 and grad.dtype == torch.bfloat16
    torch.testing.assert_close(loss.cpu().double(), ref_loss, rtol=2e-2, atol=1e-3)
    torch.testing.assert_close(grad.cpu().double(), ref_grad, rtol=2e-2, atol=2e-3)
    g = grad.cpu().float()
    assert torch.equal(g[miss], torch.zeros_like(g[miss]))
    # the tier above is absolute and the gradients shrink with 1/(Mp*cnt):
    # relative to the largest reference entry they must still agree
    scale = float(ref_grad.abs().max())
    if scale > 0:
        assert float((g.double() - ref_grad).abs().max()) <= 2e-2 * scale


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_no_nan_equals_dense_op(dev, shape):
    from deeprest_amd.ops import pinball_loss

    out, y, _, _, _ = _case(shape, "none")
    q = _quantiles(shape[3])
    loss, grad = _run(dev, out, y, q)
    o = out.to(dev).requires_grad_(True)
    dense = pinball_loss(o, y.to(dev), q)
    dense.backward()
    torch.testing.assert_close(loss, dense.detach(), **_loss_tol(shape))
    torch.testing.assert_close(grad, o.grad, rtol=1e-5, atol=1e-7)


# -------------------------------------------------------------- 2. poison
POISON_CASES = ([(s, torch.float32) for s in SHAPES]
                + [(s, torch.bfloat16) for s in BF16_SHAPES])


@pytest.mark.parametrize("pattern", ["random40", "one_metric", "all"])
@pytest.mark.parametrize("shape,dtype", POISON_CASES, ids=str)
def test_poison_at_missing_positions_changes_nothing(dev, shape, dtype, pattern):
    """NaN and +-Inf in ``outputs`` at the missing positions, and Inf instead
    of NaN as the label marker, leave the gradients bit for bit as they are.

    The loss is compared bit for bit where one block owns each metric's rows
    (at most 256 labels in all: whatever the row-lane count, a single flush per
    metric).  Larger shapes add one partial per block with float atomics, whose
    order is not fixed from launch to launch, so two runs of the SAME inputs
    may differ in the last bits; there the loss must agree within the f32
    summation bound, and any leak of a NaN/Inf would break that too."""
    out, y, miss, _, _ = _case(shape, pattern, dtype)
    q = _quantiles(shape[3])
    loss, grad = _run(dev, out, y, q)

    poison = torch.tensor([float("nan"), float("inf"), float("-inf")])
    idx = miss.nonzero(as_tuple=False)
    bad_out = out.clone().float()
    fill = poison[torch.arange(len(idx)) % 3].unsqueeze(-1).expand(-1, shape[3])
    bad_out[miss] = fill
    bad_out = bad_out.to(dtype)
    bad_y = y.clone()
    marker = torch.tensor([float("inf"), float("-inf"), float("nan")])
    bad_y[miss] = marker[torch.arange(len(idx)) % 3]
    assert not torch.isfinite(bad_out[miss]).any()

    loss_p, grad_p = _run(dev, bad_out, bad_y, q)
    assert torch.equal(grad_p, grad)
    B, T, M, _ = shape
    if B * T * M <= 256:
        assert torch.equal(loss_p, loss)
    else:
        torch.testing.assert_close(loss_p, loss, **_loss_tol(shape))


# ------------------------------------------------------------- 3. capture
def test_captured_forward_backward_follows_the_mask(dev):
    from deeprest_amd.ops import masked_pinball_loss

    shape = (4, 12, 9, 3)
    cases = [_case(shape, "random40", seed=1), _case(shape, "one_metric", seed=2),
             _case(shape, "random40", seed=3)]
    out0, y0 = cases[0][0], cases[0][1]
    static_out = out0.to(dev).requires_grad_(True)
    static_y = torch.rand(*shape[:3], device=dev)          # nothing missing yet

    def step():
        loss = masked_pinball_loss(static_out, static_y, QUANTILES)
        loss.backward()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    static_out.grad = None      # backward inside the capture allocates the static grad

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static_loss = step()

    for out, y, miss, ref_loss, ref_grad in cases:
        with torch.no_grad():
            static_out.copy_(out.to(dev))
        static_y.copy_(y.to(dev))
        static_out.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        torch.testing.assert_close(static_loss.detach().cpu().double(), ref_loss,
                                   **_loss_tol(shape))
        g = static_out.grad.cpu()
        torch.testing.assert_close(g.double(), ref_grad, rtol=1e-5, atol=1e-7)
        assert torch.equal(g[miss], torch.zeros_like(g[miss]))
    assert cases[1][2][:, :, shape[2] - 1].all()            # a metric was emptied


# --------------------------------------------------------------- 4. model
@pytest.fixture(scope="module")
def model_setup(dev):
    from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
    from deeprest_amd.models.net import build_model_spec

    app = SyntheticApp(SyntheticAppConfig(
        n_apis=8, n_components=8, windows_per_day=120, n_days=1, seed=11))
    spec = build_model_spec(app.generate_featurized())
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(4, 30, spec.num_paths, generator=gen)
    ys = []
    for _ in range(3):
        y = torch.rand(4, 30, spec.num_metrics, generator=gen)
        y[torch.rand(4, 30, spec.num_metrics, generator=gen) < 0.3] = float("nan")
        ys.append(y.to(dev))
    return spec, x.to(dev), ys


def _model(spec, dev):
    from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig

    torch.manual_seed(3)
    return DeepRestNet(spec, DeepRestNetConfig(
        d_model=64, n_heads=2, n_layers=1, d_ff=128, hidden=128, comp_dim=16,
        dropout=0.0)).to(dev)


def test_train_step_with_nan_labels(dev, model_setup):
    from deeprest_amd.engine.step import TrainStep
    from deeprest_amd.ops.adam import FusedAdam

    spec, x, ys = model_setup
    model = _model(spec, dev)
    opt = FusedAdam(model.parameters(), lr=1e-3)
    step = TrainStep(model, opt,
                     loss_fn=lambda o, t: model.loss(o, t, missing=True),
                     autocast_dtype=torch.bfloat16)
    before = [p.detach().clone() for p in model.parameters()]
    assert torch.isnan(ys[0]).any()
    loss = step(x, ys[0])
    assert torch.isfinite(loss).item(), float(loss)
    for p in model.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    changed = [not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters())]
    assert any(changed) and all(torch.isfinite(p).all() for p in model.parameters())
    # the dense loss on the same labels is what this replaces
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        assert torch.isnan(model.loss(model(x), ys[0]))


def test_graphed_train_step_with_changing_nan_labels(dev, model_setup):
    """The captured step (engine/graphstep.py) with NaN labels staged into
    static_y: each replay follows that batch's own mask."""
    from deeprest_amd.engine.step import TrainStep
    from deeprest_amd.ops.adam import FusedAdam

    spec, x, ys = model_setup
    model = _model(spec, dev)
    opt = FusedAdam(model.parameters(), lr=1e-3, capturable=True)
    step = TrainStep(model, opt,
                     loss_fn=lambda o, t: model.loss(o, t, missing=True),
                     autocast_dtype=torch.bfloat16)
    assert step.try_capture(x, ys[0], warmup=2), "capture failed"
    # one metric of the last batch is never observed
    ys = list(ys)
    ys[2] = ys[2].clone()
    ys[2][:, :, 0] = float("nan")
    losses = [step(x, y).detach().clone() for y in ys]
    torch.cuda.synchronize()
    assert all(np.isfinite([float(l) for l in losses])), losses
    assert all(torch.isfinite(p).all() for p in model.parameters())
