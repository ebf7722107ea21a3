"""GPU tests of ops.fused_gru_decode: the inference GRU kernel that projects
each step's hidden state onto the quantile heads itself
(gru_fwd_kernel<*, false, *, *, HEADS>) and never writes h_all, and of the
model flag cfg.fused_head_decode that routes forward / forward_long through
it.

The reference is the EXISTING kernel, not the code under test:
``h_all = fused_gru_sequence(...)`` with the same fp8 flag, ``ref = h_all @
w_head^T`` in fp32 and ``S = |h_all| @ |w_head|^T``.

Output bound ``|out - ref| <= 2^-7 * S + 1e-6``: the recurrence is untouched
and the head phase reads exactly the values h_all holds, so the only new
error is one bf16 rounding (unit roundoff 2^-8) — of w_head for f32 inputs,
of the output for bf16 ones — at most 2^-8 * S, plus fp32 accumulation order
(~128 * 2^-24 * S), with a 2x margin.

h_last: bit-identical to h_all[:, last] in bf16 (same fp32 state, same
rounding); for f32 / fp8 inputs h_all holds the bf16- / e4m3-rounded mirror
while h_last is the unrounded state, so they differ by one rounding: 2^-8
relative for bf16, 2^-4 relative + 2^-10 (subnormal half-spacing) for e4m3
(|h| < 1: no saturation).
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

H = 128

# (B, T, C, O) — the shapes of test_gru_heads_gpu.py, each the smallest that
# reaches its branch
SMALL = [
    (3, 7, 5, 9),      # 4-wave kernel (NSUB=1), baseline
    (2, 1, 3, 9),      # T=1
    (5, 4, 13, 9),     # R=65: ragged last 64-row tile
    (3, 5, 4, 1),      # O=1
    (3, 5, 4, 8),      # half an N-tile
    (3, 5, 4, 16),     # exactly one N-tile (the second is skipped)
    (3, 5, 4, 17),     # one column into the second
    (3, 5, 4, 32),     # both N-tiles full
]
LARGE = [
    (400, 3, 64, 9),   # 200 128-row tiles: 8-wave kernel (NSUB=2)
    (3080, 2, 8, 15),  # NSUB=2 with a ragged tail block and odd O
]
BF16_SHAPES = [SMALL[0], SMALL[6]] + LARGE
FP8_SHAPES = [SMALL[0], SMALL[2], SMALL[7]]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeprest_amd.ops import native_available

    if not native_available():
        pytest.fail("HIP extension not built — GPU tests must not fall back")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _release_shared_cases():
    """The shared references live on the device; drop them with the module."""
    yield
    _case.cache_clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _inputs(shape, dtype):
    B, T, C, O = shape
    gen = torch.Generator().manual_seed(1000 * B + 100 * T + 10 * C + O)
    mk = lambda *s: torch.randn(*s, generator=gen) * 0.4
    ins = [mk(B, T, 3 * H), mk(3 * H, H) / H ** 0.5, mk(3 * H) * 0.2,
           mk(B, C, H), 1.0 + 0.1 * mk(C, 3 * H), 0.1 * mk(C, 3 * H),
           mk(O, H) / H ** 0.5]
    # b_hh stays fp32 (the op takes it as such); the rest carry the dtype
    return [t if i == 2 else t.to(dtype) for i, t in enumerate(ins)]


def _ref_from(h_all, w_head):
    ref = h_all.float() @ w_head.float().t()
    S = h_all.float().abs() @ w_head.float().abs().t()
    return ref, S


@functools.lru_cache(maxsize=None)
def _case(shape, reverse, dtype, fp8):
    """Inputs on the device and the existing kernel's result, computed once
    per (shape, direction, dtype, fp8) and shared by the tests below."""
    from deeprest_amd.ops import fused_gru_sequence

    dev = torch.device("cuda:0")
    ins = [t.to(dev) for t in _inputs(shape, dtype)]
    with torch.no_grad():
        h_all = fused_gru_sequence(*ins[:6], reverse=reverse, fp8=fp8)
    return ins, h_all, _ref_from(h_all, ins[6])


def _check_out(out, ref, S, what):
    assert out.shape == ref.shape, what
    assert torch.isfinite(out).all(), what
    excess = (out.float() - ref).abs() - (2.0 ** -7 * S + 1e-6)
    print(f"{what}: max |out-ref| {(out.float() - ref).abs().max().item():.3e}, "
          f"max bound {(2.0 ** -7 * S).max().item():.3e}, "
          f"max excess {excess.max().item():.3e}")
    assert excess.max().item() <= 0, what


def _check_h_last(h_last, h_all, reverse, dtype, fp8, what):
    last = h_all[:, 0 if reverse else -1]
    assert h_last.shape == last.shape and h_last.dtype == last.dtype, what
    if dtype == torch.bfloat16 and not fp8:
        assert torch.equal(h_last, last), what
        return
    diff = (h_last.float() - last.float()).abs()
    if fp8:
        bound = 2.0 ** -4 * h_last.float().abs() + 2.0 ** -10
    else:
        bound = 2.0 ** -8 * h_last.float().abs()
    print(f"{what}: max h_last excess {(diff - bound).max().item():.3e}")
    assert (diff <= bound).all(), what


def _run_case(shape, reverse, dtype, fp8):
    from deeprest_amd.ops import fused_gru_decode

    ins, h_all, (ref, S) = _case(shape, reverse, dtype, fp8)
    with torch.no_grad():
        out, h_last = fused_gru_decode(*ins, reverse=reverse, fp8=fp8)
    what = f"{shape} rev={reverse} {dtype} fp8={fp8}"
    assert out.dtype == dtype and out.is_contiguous()
    _check_out(out, ref, S, what)
    _check_h_last(h_last, h_all, reverse, dtype, fp8, what)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", SMALL + LARGE)
def test_f32_matches_existing_kernel(dev, shape, reverse):
    _run_case(shape, reverse, torch.float32, False)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", BF16_SHAPES)
def test_bf16_matches_existing_kernel(dev, shape, reverse):
    _run_case(shape, reverse, torch.bfloat16, False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", FP8_SHAPES)
def test_fp8_matches_existing_kernel(dev, shape, reverse, dtype):
    _run_case(shape, reverse, dtype, True)


@pytest.mark.parametrize("reverse", [False, True])
def test_chunk_carry_bf16(dev, reverse):
    """T = 7 split 4 + 3: decode carried through h_last against the unfused
    op carried through h_all[:, last] — bit-equal states at the boundary, and
    the concatenated out within the output bound of the unfused chunks."""
    from deeprest_amd.ops import fused_gru_decode, fused_gru_sequence

    shape = SMALL[0]
    xg, w_hh, b_hh, h0, gamma, beta, w_head = [
        t.to(dev) for t in _inputs(shape, torch.bfloat16)]
    pieces = [slice(0, 4), slice(4, 7)]
    if reverse:
        pieces.reverse()
    h_dec, h_ref = h0, h0
    outs, refs, Ss = [], [], []
    with torch.no_grad():
        for sl in pieces:
            x = xg[:, sl].contiguous()
            out, h_dec = fused_gru_decode(x, w_hh, b_hh, h_dec, gamma, beta,
                                          w_head, reverse=reverse)
            h_all = fused_gru_sequence(x, w_hh, b_hh, h_ref, gamma, beta,
                                       reverse=reverse)
            h_ref = h_all[:, 0 if reverse else -1].contiguous()
            assert torch.equal(h_dec, h_ref), f"carried state differs at {sl}"
            ref, S = _ref_from(h_all, w_head)
            outs.append(out), refs.append(ref), Ss.append(S)
    if reverse:
        outs.reverse(), refs.reverse(), Ss.reverse()
    _check_out(torch.cat(outs, 1), torch.cat(refs, 1), torch.cat(Ss, 1),
               f"chunked rev={reverse}")


def test_raises_when_grad_is_required(dev):
    from deeprest_amd.ops import fused_gru_decode

    ins = [t.to(dev) for t in _inputs(SMALL[0], torch.float32)]
    ins[1].requires_grad_(True)
    with pytest.raises(RuntimeError):
        fused_gru_decode(*ins)


def test_binding_rejects_bad_head_images(dev):
    """The kernel entry refuses an O its two N-tiles cannot hold and a weight
    image of the wrong shape or dtype (it would read outside the image); both
    forward entries refuse operands whose shapes or device do not match
    x_gates."""
    from deeprest_amd.ops.native import require_native

    ext = require_native("test")
    xg, w_hh, b_hh, h0, gamma, beta, _ = [
        t.to(dev) for t in _inputs((2, 2, 3, 9), torch.float32)]
    img = torch.zeros(32, H, device=dev, dtype=torch.bfloat16)
    args = (xg, w_hh, b_hh, h0, gamma, beta)
    for bad_img, bad_o in [(img, 33), (img, 0), (img[:16].contiguous(), 9),
                           (img.float(), 9)]:
        with pytest.raises(RuntimeError):
            ext.gru_seq_decode(*args, bad_img, bad_o, False, False)

    # the sequence entry shares the decode entry's operand checks: a short
    # h0 / beta / b_hh or a host tensor never reaches the kernel
    B, T, C = 2, 3, 3
    good = dict(zip(("xg", "w_hh", "b_hh", "h0", "gamma", "beta"), (
        t.to(dev) for t in _inputs((B, T, C, 9), torch.float32)[:6])))
    bad_operands = {
        "h0 of batch B + 1": {"h0": torch.cat([good["h0"], good["h0"][:1]])},
        "beta one row short": {"beta": good["beta"][:-1].contiguous()},
        "b_hh of 3H - 1": {"b_hh": good["b_hh"][:-1].contiguous()},
        "h0 on the host": {"h0": good["h0"].cpu()},
    }
    for what, swap in bad_operands.items():
        print("gru_seq_forward with", what)
        with pytest.raises(RuntimeError):
            ext.gru_seq_forward(*{**good, **swap}.values(), False, False)
    h_all, _ = ext.gru_seq_forward(*good.values(), False, False)
    assert h_all.shape == (B, T, C, H)


# -------------------------------------------------------------------- model
def _spec(n_components):
    from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
    from deeprest_amd.models.net import build_model_spec

    app = SyntheticApp(SyntheticAppConfig(
        n_apis=5, n_components=n_components, windows_per_day=120, n_days=1,
        seed=23))
    return build_model_spec(app.generate_featurized())


def _model(spec, decode, dev, fp8=False, seed=4):
    from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig

    torch.manual_seed(seed)
    return DeepRestNet(spec, DeepRestNetConfig(
        d_model=64, n_heads=2, n_layers=1, d_ff=128, hidden=128, comp_dim=16,
        dropout=0.0, fused_head_decode=decode, fp8_inference=fp8)).to(dev)


@pytest.fixture
def decode_calls(monkeypatch):
    """Counts calls of the decode op as the model sees it."""
    from deeprest_amd.models import net

    calls = []
    real = net.fused_gru_decode

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(net, "fused_gru_decode", counted)
    return calls


def test_model_forward_and_forward_long(dev, decode_calls):
    spec = _spec(6)
    off = _model(spec, False, dev).eval()
    on = _model(spec, True, dev).eval()
    on.load_state_dict(off.state_dict())
    x = torch.rand(2, 96, spec.num_paths, device=dev)
    with torch.no_grad():
        full_off = off(x)
        assert len(decode_calls) == 0
        full_on = on(x)
        assert len(decode_calls) == 2          # once per direction
        long_on = on.forward_long(x, chunk_size=96)
        multi_on = on.forward_long(x, chunk_size=32)
    torch.testing.assert_close(full_on, full_off, rtol=5e-2, atol=3e-2)
    torch.testing.assert_close(long_on, full_on, rtol=2e-4, atol=2e-4)
    assert multi_on.shape == full_on.shape and torch.isfinite(multi_on).all()

    on.cfg.fp8_inference = True
    with torch.no_grad():
        fp8_on = on(x)
        fp8_long_on = on.forward_long(x, chunk_size=96)
    for name, got in [("forward", fp8_on), ("forward_long", fp8_long_on)]:
        err = (got - full_off).abs().max().item()
        print(f"fp8 {name} flag-on vs non-fp8 forward: max abs err {err:.4f}")
        assert err < 0.5, f"fp8 decode drifted ({name}): {err}"
    torch.testing.assert_close(fp8_long_on, fp8_on, rtol=2e-4, atol=2e-4)


def _train_step(spec, decode, dev, x, y):
    model = _model(spec, decode, dev, seed=3).train()
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        out = model(x)
        loss = model.loss(out.float(), y)
    loss.backward()
    return (out.detach(), loss.detach(),
            {n: p.grad for n, p in model.named_parameters()})


def test_training_mode_ignores_the_flag(dev, decode_calls):
    """Training step with the flag on: the decode route is inference-only, so
    the op is never called and the step is the flag-off model's.

    The predictions are bit-equal.  The loss and the gradients cannot be
    asked to be: the pinball loss and several backward reductions (LayerNorm
    weights, GRU dgamma / dbeta / b_hh) finish with fp32 atomics in arbitrary
    order, and two runs of the SAME flag-off step on one device already
    differ in the last bits (measured: 6e-8 in a loss of 0.79; 2e-9 in
    in_norm.weight with max 2.6e-2; 6e-11 in decoder.b_hh_r with max 2.9e-2)
    — for some parameters in one pair of runs and not in the next.  Their
    bounds therefore come from the number formats:
    - loss: a sum of at most 2^11 non-negative per-block partials (the
      kernel's grid cap), so any order is within 2^11 * 2^-24 = 2^-13
      relative;
    - gradients: a different accumulation order moves an fp32 sum by far less
      than that and can at most flip the rounding of the bf16 gradient
      tensors it flows through, one bf16 rounding of the largest entry:
      2^-8 * max|grad|."""
    spec = _spec(6)
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(4, 30, spec.num_paths, generator=gen).to(dev)
    y = torch.rand(4, 30, spec.num_metrics, generator=gen).to(dev)
    out_off, loss_off, g_off = _train_step(spec, False, dev, x, y)
    out_on, loss_on, g_on = _train_step(spec, True, dev, x, y)
    assert len(decode_calls) == 0
    assert torch.equal(out_on, out_off)
    print(f"loss off {loss_off.item():.9g}, flag-on diff "
          f"{(loss_on - loss_off).abs().item():.3e}")
    assert (loss_on - loss_off).abs() <= 2.0 ** -13 * loss_off.abs()
    assert g_on.keys() == g_off.keys()
    failed = []
    for name in g_off:
        assert (g_on[name] is None) == (g_off[name] is None), name
        if g_off[name] is None:
            continue
        scale = g_off[name].abs().max().item()
        err = (g_on[name] - g_off[name]).abs().max().item()
        if err > 0:
            print(f"{name}: flag-on diff {err:.3e}, max|grad| {scale:.3e}")
        if err > 2.0 ** -8 * scale:
            failed.append(name)
    assert not failed, failed


def test_forward_long_memory(dev):
    """forward_long with the flag off must retain every chunk's (1, Tc, C, H)
    hidden sequence per direction until the end; with the flag on nothing
    H-wide outlives a chunk.  The peak must drop by at least half of that
    retained h_all (the other half is margin for what both paths hold)."""
    spec = _spec(15)
    C, T, dirs = spec.num_components, 4096, 2
    assert C == 16
    off = _model(spec, False, dev).eval()
    on = _model(spec, True, dev).eval()
    on.load_state_dict(off.state_dict())
    x = torch.rand(1, T, spec.num_paths, device=dev)
    peaks = {}
    for name, model in (("off", off), ("on", on)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        with torch.no_grad():
            out = model.forward_long(x, chunk_size=512)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated()
        assert torch.isfinite(out).all()
        del out
    need = 0.5 * dirs * T * C * H * 4
    print(f"peak off {peaks['off']} B, on {peaks['on']} B, "
          f"saved {peaks['off'] - peaks['on']} B, required {need:.0f} B")
    assert peaks["off"] - peaks["on"] >= need
