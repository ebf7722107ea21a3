"""GPU tests of ``ops.mha_packed``: attention on the packed qkv projection.

The reference is always ``reference_mha`` in fp32 on the unpacked views of the
same (IO-dtype-rounded) input, with its autograd for the gradients; never the
(B, H, T, D) kernel path and never the code under test.  Tolerances are the
tiers of ``test_ops_gpu.py``: forward rtol 3e-2 / atol 2e-2, gradients
rtol 5e-2 / atol 3e-2.

T <= 64 with Dh in {16, 32, 64} runs the whole-head tile kernels, everything
else the flash-style bodies on the packed strides.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = dict(rtol=3e-2, atol=2e-2)
GRAD_TOL = dict(rtol=5e-2, atol=3e-2)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeprest_amd.ops import native_available

    if not native_available():
        pytest.fail("HIP extension not built — GPU tests must not fall back")
    return torch.device("cuda:0")


def _reference(qkv, n_heads, d_out):
    """fp32 reference_mha on the unpacked views: (o, dqkv) in fp32."""
    from deeprest_amd.ops import reference_mha

    B, T = qkv.shape[:2]
    x = qkv.detach().float().reshape(B, T, 3, n_heads, -1).requires_grad_(True)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    o = reference_mha(q, k, v).transpose(1, 2).reshape(B, T, -1)
    o.backward(d_out.float())
    return o.detach(), x.grad.reshape(qkv.shape)


def _run(qkv, n_heads, d_out):
    from deeprest_amd.ops import mha_packed

    x = qkv.detach().requires_grad_(True)
    o = mha_packed(x, n_heads)
    o.backward(d_out)
    return o.detach(), x.grad


# the reference of a (T, BH, Dh, dtype) case is computed once
_REF_CACHE = {}


def _case(dev, T, B, H, Dh, dtype):
    key = (T, B, H, Dh, dtype)
    if key not in _REF_CACHE:
        gen = torch.Generator(device="cpu").manual_seed(1000 * T + 10 * Dh + B)
        qkv = (0.7 * torch.randn(B, T, 3 * H * Dh, generator=gen)).to(dev, dtype)
        d_out = (0.7 * torch.randn(B, T, H * Dh, generator=gen)).to(dev, dtype)
        _REF_CACHE[key] = (qkv, d_out) + _reference(qkv, H, d_out)
    return _REF_CACHE[key]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("Dh", [8, 16, 32, 64])
@pytest.mark.parametrize("BH", [(2, 3), (37, 8)], ids=["2x3", "37x8"])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 33, 60, 64, 65, 128])
def test_packed_matches_reference(dev, T, BH, Dh, dtype):
    B, H = BH
    qkv, d_out, o_ref, g_ref = _case(dev, T, B, H, Dh, dtype)
    o, g = _run(qkv, H, d_out)
    assert o.shape == (B, T, H * Dh) and o.is_contiguous() and o.dtype == dtype
    assert g.shape == qkv.shape and g.dtype == dtype
    print(f"T={T} BH={BH} Dh={Dh} {dtype}: max |o - ref| "
          f"{(o.float() - o_ref).abs().max().item():.3e}, max |dqkv - ref| "
          f"{(g.float() - g_ref).abs().max().item():.3e} "
          f"(max |ref| {g_ref.abs().max().item():.3e})")
    torch.testing.assert_close(o.float(), o_ref, **FWD_TOL)
    torch.testing.assert_close(g.float(), g_ref, **GRAD_TOL)


def test_packed_takes_the_5d_shape(dev):
    qkv, d_out, o_ref, g_ref = _case(dev, 60, 2, 3, 32, torch.bfloat16)
    o, g = _run(qkv.view(2, 60, 3, 3, 32), 3, d_out)
    assert g.shape == (2, 60, 3, 3, 32)
    o3, g3 = _run(qkv, 3, d_out)
    assert torch.equal(o, o3) and torch.equal(g.view_as(g3), g3)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_packed_asymmetric_catches_transpose(dev, dtype):
    """q and k are one ramp column each, v and dO are arange * 0.01: a swapped
    row / column or a wrong k permutation of an accumulator-fed MFMA operand is
    a large error, not noise.  Forward at the tolerance of
    test_mha_asymmetric_catches_transpose.  The gradients reach magnitudes in
    the hundreds here, so they are bounded relative to each part's scale: P and
    dS are rounded to bf16 (2^-9 relative each) before products of up to 33
    terms of one sign, and for f32 IO the operands are too; 2e-2 of the largest
    reference element is the project's relative-to-scale bound and ten times
    that rounding, while a permuted operand is wrong by the scale itself."""
    T, Dh = 33, 32
    qkv = torch.zeros(1, T, 3, 1, Dh, device=dev)
    qkv[0, :, 0, 0, 0] = torch.arange(T, device=dev) * 0.1
    qkv[0, :, 1, 0, 0] = torch.arange(T, device=dev) * 0.05
    qkv[0, :, 2, 0, :] = torch.arange(T * Dh, device=dev).reshape(T, Dh) * 0.01
    d_out = (torch.arange(T * Dh, device=dev).reshape(1, T, Dh) * 0.01).to(dtype)
    qkv = qkv.reshape(1, T, 3 * Dh).to(dtype)
    o_ref, g_ref = _reference(qkv, 1, d_out)
    o, g = _run(qkv, 1, d_out)
    torch.testing.assert_close(o.float(), o_ref, rtol=2e-2, atol=2e-2)
    g = g.float().view(T, 3, Dh)
    g_ref = g_ref.view(T, 3, Dh)
    for i, name in enumerate(("dq", "dk", "dv")):
        err = (g[:, i] - g_ref[:, i]).abs().max().item()
        mag = g_ref[:, i].abs().max().item()
        print(f"asymmetric {dtype} {name}: max err {err:.3e}, max |ref| {mag:.3e}")
        assert err <= 2e-2 * mag, (name, err, mag)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("Dh", [16, 32, 64])
def test_packed_ignores_what_surrounds_the_tensors(dev, Dh, dtype):
    """qkv and dO as views into NaN-filled buffers (batches before and after;
    rows >= T of the last head tile fall into the guard): bit-identical to the
    same call on clean copies."""
    B, H, T = 3, 3, 60
    qkv, d_out, _, _ = _case(dev, T, B, H, Dh, dtype)
    big = torch.full((B + 2, T, 3 * H * Dh), float("nan"), device=dev, dtype=dtype)
    big[1:B + 1] = qkv
    big_do = torch.full((B + 2, T, H * Dh), float("nan"), device=dev, dtype=dtype)
    big_do[1:B + 1] = d_out
    o_clean, g_clean = _run(qkv.clone(), H, d_out.clone())
    o, g = _run(big[1:B + 1], H, big_do[1:B + 1])
    assert torch.isfinite(o_clean.float()).all() and torch.isfinite(g_clean.float()).all()
    assert torch.equal(o, o_clean)
    assert torch.equal(g, g_clean)
    # and nothing was written around them
    assert torch.isnan(big[0]).all() and torch.isnan(big[-1]).all()
    assert torch.isnan(big_do[0]).all() and torch.isnan(big_do[-1]).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("Dh", [16, 32, 64])
@pytest.mark.parametrize("T", [17, 60, 64])
def test_whole_tile_path_is_exact_under_rolls_and_repeats(dev, T, Dh, dtype):
    """No atomics on the whole-tile path: heads are independent and the op is
    deterministic, bit for bit."""
    B, H = 5, 3
    qkv, d_out, _, _ = _case(dev, T, B, H, Dh, dtype)
    o, g = _run(qkv, H, d_out)
    o2, g2 = _run(qkv, H, d_out)
    assert torch.equal(o, o2) and torch.equal(g, g2)
    # batch rolled by one
    o_b, g_b = _run(qkv.roll(1, 0), H, d_out.roll(1, 0))
    assert torch.equal(o_b, o.roll(1, 0)) and torch.equal(g_b, g.roll(1, 0))
    # heads rolled by one
    q5 = qkv.view(B, T, 3, H, Dh).roll(1, 3).reshape(B, T, -1).contiguous()
    d4 = d_out.view(B, T, H, Dh).roll(1, 2).reshape(B, T, -1).contiguous()
    o_h, g_h = _run(q5, H, d4)
    assert torch.equal(o_h.view(B, T, H, Dh), o.view(B, T, H, Dh).roll(1, 2))
    assert torch.equal(g_h.view(B, T, 3, H, Dh), g.view(B, T, 3, H, Dh).roll(1, 3))


def test_packed_off_is_the_old_composition(dev):
    """PACKED_MODE "off" runs views + mha_forward + reshape; both modes meet the
    reference."""
    from deeprest_amd.ops import attention

    qkv, d_out, o_ref, g_ref = _case(dev, 60, 2, 3, 32, torch.bfloat16)
    assert attention.PACKED_MODE == "auto"
    attention.PACKED_MODE = "off"
    try:
        o, g = _run(qkv, 3, d_out)
    finally:
        attention.PACKED_MODE = "auto"
    torch.testing.assert_close(o.float(), o_ref, **FWD_TOL)
    torch.testing.assert_close(g.float(), g_ref, **GRAD_TOL)


# ---------------------------------------------------------------- the binding
def test_binding_rejects_bad_operands(dev):
    from deeprest_amd.ops import mha_packed

    good = torch.randn(2, 16, 3 * 2 * 32, device=dev, dtype=torch.bfloat16)
    mha_packed(good, 2)
    with pytest.raises(RuntimeError, match="contiguous"):
        mha_packed(torch.randn(2, 16, 2 * 3 * 2 * 32, device=dev)[:, :, ::2], 2)
    with pytest.raises(RuntimeError, match="last dimension"):
        mha_packed(torch.randn(2, 16, 3 * 2 * 32 + 8, device=dev), 2)
    with pytest.raises(RuntimeError, match="head dim"):
        mha_packed(torch.randn(2, 16, 3 * 2 * 12, device=dev), 2)
    with pytest.raises(RuntimeError, match="bf16 or f32"):
        mha_packed(torch.zeros(2, 16, 3 * 2 * 32, device=dev, dtype=torch.int32), 2)
    with pytest.raises(RuntimeError, match="n_heads"):
        mha_packed(torch.randn(2, 16, 3, 4, 32, device=dev), 2)


# ------------------------------------------------------------------ the model
def _model_and_data(dev, fused):
    from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
    from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig, build_model_spec

    app = SyntheticApp(SyntheticAppConfig(
        n_apis=8, n_components=8, windows_per_day=120, n_days=1, seed=11))
    spec = build_model_spec(app.generate_featurized())
    torch.manual_seed(3)
    model = DeepRestNet(spec, DeepRestNetConfig(
        d_model=64, n_heads=2, n_layers=1, d_ff=128, hidden=128, comp_dim=16,
        dropout=0.0, fused_residual_norm=fused)).to(dev)
    gen = torch.Generator(device="cpu").manual_seed(4)
    x = torch.randn(4, 30, spec.num_paths, generator=gen).to(dev)
    y = torch.rand(4, 30, spec.num_metrics, generator=gen).to(dev)
    return model, x, y


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused_residual_norm"])
def test_model_packed_against_off(dev, fused):
    from deeprest_amd.ops import attention

    results = {}
    for mode in ("auto", "off"):
        model, x, y = _model_and_data(dev, fused)
        attention.PACKED_MODE = mode
        try:
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                out = model(x)
                loss = model.loss(out.float(), y)
            loss.backward()
        finally:
            attention.PACKED_MODE = "auto"
        results[mode] = (out.detach().float(),
                         {n: p.grad.float() for n, p in model.named_parameters()
                          if p.grad is not None})
    out_a, grads_a = results["auto"]
    out_o, grads_o = results["off"]
    torch.testing.assert_close(out_a, out_o, **FWD_TOL)
    assert grads_a.keys() == grads_o.keys() and grads_a
    for name in grads_a:
        torch.testing.assert_close(grads_a[name], grads_o[name], **GRAD_TOL, msg=name)


def test_model_with_lengths_is_untouched(dev):
    from deeprest_amd.ops import attention

    outs = []
    lengths = torch.tensor([30, 7, 19, 1], dtype=torch.int32, device=dev)
    for mode in ("auto", "off"):
        model, x, _ = _model_and_data(dev, False)
        model.eval()
        attention.PACKED_MODE = mode
        try:
            with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                outs.append(model(x, lengths=lengths))
        finally:
            attention.PACKED_MODE = "auto"
    assert torch.equal(outs[0], outs[1])
