"""GPU tests of the wave-owned forward time loop of gru_fwd_kernel and of the
head projection inside the training forward (SAVE && HEADS).

Each wave stages x_gates for its own 16 rows into its own LDS slots and stores
its own h_all rows, with no workgroup barrier per step, so what can go wrong is
the slot and row indexing.  The shapes (B, T, C) are the smallest that reach
each branch:

  (22, 3, 3)     4-wave; a wave spans 6 batches; ragged last tile (R = 66)
  (7, 2, 11)     4-wave; slots straddle unevenly
  (4890, 2, 5)   8-wave (192 tiles of 128 rows); 4 batches per wave; ragged
  (3500, 2, 7)   8-wave; uneven straddle
  (400, 3, 64)   8-wave; the flagship's C

Tolerances: the forward against the fp32 reference uses the GRU tier of
test_ops_gpu.py (rtol 5e-2, atol 3e-2), gradients the tiers of
test_gru_heads_gpu.py.  The comparisons of the kernel with itself are exact.
The in-kernel head output and F.linear on the same h_all are the fp32 sum of
the same 128 bf16 products in another order, rounded once, so they may differ
by one bf16 ulp of the larger value plus 1e-5 of the sum of magnitudes.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

H = 128
WAVE4 = [(22, 3, 3), (7, 2, 11)]
WAVE8 = [(4890, 2, 5), (3500, 2, 7), (400, 3, 64)]
NAMES = ["x_gates", "w_hh", "b_hh", "h0", "gamma", "beta", "w_head"]


@pytest.fixture(scope="module")
def ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeprest_amd.ops import native_available
    from deeprest_amd.ops.native import require_native

    if not native_available():
        pytest.fail("HIP extension not built — GPU tests must not fall back")
    return require_native("test_gru_fwd_wave_gpu")


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype):
    """(x_gates, w_hh, b_hh, h0, gamma, beta) on the device; b_hh stays fp32."""
    B, T, C = shape
    gen = torch.Generator().manual_seed(1000 * B + 100 * T + C)
    mk = lambda *s: torch.randn(*s, generator=gen) * 0.4
    ins = [mk(B, T, 3 * H), mk(3 * H, H) / H ** 0.5, mk(3 * H) * 0.2,
           mk(B, C, H), 1.0 + 0.1 * mk(C, 3 * H), 0.1 * mk(C, 3 * H)]
    return tuple((t if i == 2 else t.to(dtype)).cuda().contiguous()
                 for i, t in enumerate(ins))


@functools.lru_cache(maxsize=None)
def _w_head(O, dtype):
    gen = torch.Generator().manual_seed(77 + O)
    return (torch.randn(O, H, generator=gen) * 0.4 / H ** 0.5).to(dtype).cuda()


@functools.lru_cache(maxsize=None)
def _saving_forward(shape, dtype, reverse):
    """(h_all, saves) of the plain saving forward, computed once and shared."""
    from deeprest_amd.ops.native import require_native

    return tuple(require_native("test").gru_seq_forward(
        *_inputs(shape, dtype), reverse, True))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", WAVE4 + WAVE8)
def test_forward_matches_reference(ext, shape, reverse, dtype):
    from deeprest_amd.ops import reference_gru_sequence

    h_all, _ = _saving_forward(shape, dtype, reverse)
    ref = reference_gru_sequence(*[t.float() for t in _inputs(shape, dtype)],
                                 reverse=reverse)
    torch.testing.assert_close(h_all.float(), ref, rtol=5e-2, atol=3e-2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", WAVE4 + WAVE8)
def test_rows_are_independent_bitwise(ext, shape, reverse, dtype):
    """The batch rolled by one: same B, hence the same kernel variant, but
    every row sits in another wave and another staging slot.  The results are
    the rolled results, bit for bit."""
    xg, w_hh, b_hh, h0, gamma, beta = _inputs(shape, dtype)
    h_all, saves = _saving_forward(shape, dtype, reverse)
    h_r, s_r = ext.gru_seq_forward(xg.roll(1, 0).contiguous(), w_hh, b_hh,
                                   h0.roll(1, 0).contiguous(), gamma, beta,
                                   reverse, True)
    assert torch.equal(h_r, h_all.roll(1, 0))
    assert torch.equal(s_r, saves.roll(1, 0))


def test_head_phase_is_decided_by_the_binding(ext):
    for B, _, C in WAVE8:
        assert ext.gru_fwd_fuses_heads(B, C, True)
        assert not ext.gru_fwd_fuses_heads(B, C, False)
    for B, _, C in WAVE4:
        assert not ext.gru_fwd_fuses_heads(B, C, True)
    # asked for where the kernel has no head phase: an error, not a fallback
    from deeprest_amd.ops.gru import _head_image_fwd

    img = _head_image_fwd(_w_head(9, torch.bfloat16))
    with pytest.raises(RuntimeError):
        ext.gru_seq_forward(*_inputs(WAVE4[0], torch.bfloat16), False, True,
                            False, img, 9)
    with pytest.raises(RuntimeError):
        ext.gru_seq_forward(*_inputs(WAVE8[2], torch.bfloat16), False, False,
                            False, img, 9)
    with pytest.raises(RuntimeError):
        ext.gru_seq_forward(*_inputs(WAVE8[2], torch.bfloat16), False, True,
                            False, img, 33)


def _bf16_ulp(x):
    """Spacing of bf16 at magnitude x (8 significant bits): 2^(floor(log2 x) - 7)."""
    _, e = torch.frexp(x)                 # x = m * 2^e, 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(x), e - 8)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("O", [1, 9, 17, 32])
@pytest.mark.parametrize("shape", WAVE8)
def test_save_heads_against_plain_save(ext, shape, O, dtype):
    """SAVE+HEADS on the same inputs: h_all and saves are those of the plain
    saving kernel, bit for bit, and out is F.linear on that h_all with the
    bf16-rounded head weights, up to the order of the fp32 sum."""
    from deeprest_amd.ops.gru import _head_image_fwd

    reverse = O in (9, 32)                # both directions over the O cases
    h_all, saves = _saving_forward(shape, dtype, reverse)
    w_bf = _w_head(O, dtype).to(torch.bfloat16)
    h2, s2, out = ext.gru_seq_forward(*_inputs(shape, dtype), reverse, True,
                                      False, _head_image_fwd(w_bf), O)
    assert torch.equal(h2, h_all)
    assert torch.equal(s2, saves)
    assert out.shape == h_all.shape[:3] + (O,) and out.dtype == h_all.dtype

    ref = F.linear(h_all, w_bf.to(dtype)).float()
    a = out.float()
    bound = (_bf16_ulp(torch.maximum(a.abs(), ref.abs()))
             + 1e-5 * F.linear(h_all.float().abs(), w_bf.float().abs()))
    diff = (a - ref).abs()
    print(f"{shape} O={O} {dtype}: {(diff > 0).float().mean().item():.3e} of "
          f"elements differ, max diff/bound {(diff / bound).max().item():.3f}")
    assert torch.isfinite(a).all()
    assert (diff <= bound).all()


def _run(fn, ins, grad, reverse):
    leaves = [t.detach().clone().requires_grad_(True) for t in ins]
    out = fn(*leaves, reverse=reverse)
    out.backward(grad)
    return out.detach().float(), [t.grad.detach().float() for t in leaves]


def _composed(xg, w_hh, b_hh, h0, gamma, beta, w_head, reverse):
    from deeprest_amd.ops import reference_gru_sequence

    return F.linear(reference_gru_sequence(xg, w_hh, b_hh, h0, gamma, beta,
                                           reverse=reverse), w_head)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", WAVE8)
def test_fused_gru_heads_gradients(ext, shape, reverse, dtype):
    """fused_gru_heads through the in-kernel head phase, against the fp32
    composition: the large-row tiers of test_gru_heads_gpu.py."""
    from deeprest_amd.ops import fused_gru_heads

    O = 9
    ins = list(_inputs(shape, dtype)) + [_w_head(O, dtype)]
    gen = torch.Generator().manual_seed(5)
    grad = torch.randn(*shape, O, generator=gen).to(dtype).cuda()
    out, grads = _run(fused_gru_heads, ins, grad, reverse)
    out_r, grads_r = _run(_composed, [t.float() for t in ins], grad.float(),
                          reverse)
    torch.testing.assert_close(out, out_r, rtol=5e-2, atol=3e-2)
    for name, g, g_r in zip(NAMES, grads, grads_r):
        assert torch.isfinite(g).all(), f"{name}: non-finite gradient"
        rel = (g - g_r).abs().max() / (g_r.abs().max() + 1e-9)
        assert rel < 2e-2, f"{name}: relmax {rel.item():.4f}"
