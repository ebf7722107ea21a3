"""GPU tests of the GRU chain kernels' streamed FiLM operands: the pi-ordered
images of gamma / beta / b_hh that the launchers build per call, the 16-byte
loads that read them in the forward and backward epilogues, and the 16-byte
x_gates reads from a wave's LDS slot.

What can go wrong is indexing: which component's image row a lane row reads
(the rows of one wave belong to different components and batches), dead rows
of a ragged last tile, and the order in which a 16-byte load is unpacked into
N-tiles.  So gamma and beta are random per (component, column) with a wide
spread (gamma = 2 randn, beta = randn) and b_hh is distinct per column: a value
from the wrong component or column moves a gate pre-activation by O(1), far
outside the tiers below.  The shapes (B, T, C) are those of
test_gru_fwd_wave_gpu.py:

  (22, 3, 3)     4-wave; R = 66, ragged last tile
  (7, 2, 11)     4-wave; uneven straddle
  (4890, 2, 5)   8-wave; 4 batches per wave; ragged
  (3500, 2, 7)   8-wave; uneven straddle
  (400, 3, 64)   8-wave; the flagship's C

Tolerances against reference_gru_sequence on the same (rounded) inputs in
fp32: forward rtol 5e-2 / atol 3e-2; gradients rtol 8e-2 / atol 5e-2 on the
4-wave shapes and max error / max magnitude < 2e-2 on the 8-wave shapes (the
tiers of test_gru_heads_gpu.py).  The comparisons of a kernel with itself
(components rolled, batch rolled) are exact.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

H = 128
O = 9
WAVE4 = [(22, 3, 3), (7, 2, 11)]
WAVE8 = [(4890, 2, 5), (3500, 2, 7), (400, 3, 64)]
SHAPES = WAVE4 + WAVE8
DTYPES = [torch.bfloat16, torch.float32]
NAMES = ["x_gates", "w_hh", "b_hh", "h0", "gamma", "beta", "w_head"]
# share of reference |h| that must stay below 0.999: with pre-activations of
# standard deviation ~1.5 (0.4 * 2 randn + randn + hh), |tanh| > 0.999 needs
# |x| > 3.8, a few per cent at the most, and h blends n with h_prev
UNSATURATED_FLOOR = 0.95


@pytest.fixture(scope="module")
def ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeprest_amd.ops import native_available
    from deeprest_amd.ops.native import require_native

    if not native_available():
        pytest.fail("HIP extension not built — GPU tests must not fall back")
    return require_native("test_gru_epilogue_gpu")


@functools.lru_cache(maxsize=None)
def _cpu_inputs(shape):
    """fp32 (x_gates, w_hh, b_hh, h0, gamma, beta, w_head), seeded on the CPU."""
    B, T, C = shape
    gen = torch.Generator().manual_seed(7000 * B + 100 * T + C)
    rn = lambda *s: torch.randn(*s, generator=gen)
    b_hh = 0.2 * rn(3 * H) + torch.linspace(-0.3, 0.3, 3 * H)   # distinct per column
    return (0.4 * rn(B, T, 3 * H), 0.4 * rn(3 * H, H) / H ** 0.5, b_hh,
            0.4 * rn(B, C, H), 2.0 * rn(C, 3 * H), rn(C, 3 * H),
            0.4 * rn(O, H) / H ** 0.5)


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype):
    """The same on the device in `dtype`; b_hh stays fp32."""
    return tuple((t if i == 2 else t.to(dtype)).cuda().contiguous()
                 for i, t in enumerate(_cpu_inputs(shape)))


@functools.lru_cache(maxsize=None)
def _lengths(shape):
    B, T, _ = shape
    return ((torch.arange(B) * 7) % T + 1).to(torch.int32).cuda()


@functools.lru_cache(maxsize=None)
def _reference(shape, dtype, reverse, varlen):
    """fp32 reference (h_all, out, h_last) on the rounded inputs; computed
    once per case and shared, never modified."""
    from deeprest_amd.ops import reference_gru_sequence

    ins = [t.float() for t in _inputs(shape, dtype)]
    h_all, h_last = reference_gru_sequence(
        *ins[:6], reverse=reverse, lengths=_lengths(shape) if varlen else None,
        return_state=True)
    return h_all, F.linear(h_all, ins[6]), h_last


def _close(got, ref, what):
    err = (got.float() - ref).abs().max().item()
    print(f"{what}: max abs err {err:.4f} (max |ref| {ref.abs().max().item():.3f})")
    torch.testing.assert_close(got.float(), ref, rtol=5e-2, atol=3e-2,
                               msg=lambda m: f"{what}: {m}")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_inputs_keep_the_reference_unsaturated(shape, reverse):
    """On the CPU: with the wide FiLM operands the reference stays finite and
    most of |h| stays off the tanh rails, so a wrong operand shows in h."""
    from deeprest_amd.ops import reference_gru_sequence

    h_all = reference_gru_sequence(*_cpu_inputs(shape)[:6], reverse=reverse)
    assert torch.isfinite(h_all).all()
    share = (h_all.abs() < 0.999).float().mean().item()
    print(f"{shape} rev={reverse}: {share:.4f} of |h| below 0.999")
    assert share >= UNSATURATED_FLOOR


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_saving_forward_matches_reference(ext, shape, reverse, dtype):
    """The saving kernel without the head phase, and with it where it exists."""
    from deeprest_amd.ops.gru import _head_image_fwd

    ins = _inputs(shape, dtype)
    ref_h, ref_out, _ = _reference(shape, dtype, reverse, False)
    h_all, _ = ext.gru_seq_forward(*ins[:6], reverse, True)
    _close(h_all, ref_h, f"{shape} save h_all")
    if ext.gru_fwd_fuses_heads(shape[0], shape[2], True):
        h2, _, out = ext.gru_seq_forward(*ins[:6], reverse, True, False,
                                         _head_image_fwd(ins[6]), O)
        _close(h2, ref_h, f"{shape} save+heads h_all")
        _close(out, ref_out, f"{shape} save+heads out")
    else:
        assert shape in WAVE4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["plain", "varlen", "fp8", "fp8_varlen"])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_decode_matches_reference(ext, shape, reverse, mode, dtype):
    from deeprest_amd.ops import fused_gru_decode

    varlen = mode.endswith("varlen")
    _, ref_out, ref_last = _reference(shape, dtype, reverse, varlen)
    with torch.no_grad():
        out, h_last = fused_gru_decode(
            *_inputs(shape, dtype), reverse=reverse, fp8=mode.startswith("fp8"),
            lengths=_lengths(shape) if varlen else None)
    _close(out, ref_out, f"{shape} {mode} out")
    _close(h_last, ref_last, f"{shape} {mode} h_last")


def _run(fn, ins, grad, reverse):
    leaves = [t.detach().clone().requires_grad_(True) for t in ins]
    out = fn(*leaves, reverse=reverse)
    out.backward(grad)
    return out.detach().float(), [t.grad.detach().float() for t in leaves]


def _ref_sequence(xg, w_hh, b_hh, h0, gamma, beta, reverse):
    from deeprest_amd.ops import reference_gru_sequence

    return reference_gru_sequence(xg, w_hh, b_hh, h0, gamma, beta, reverse=reverse)


def _ref_heads(xg, w_hh, b_hh, h0, gamma, beta, w_head, reverse):
    return F.linear(_ref_sequence(xg, w_hh, b_hh, h0, gamma, beta, reverse), w_head)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "heads"])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_matches_reference(ext, shape, reverse, fused, dtype):
    """gru_bwd_kernel through the ops: plain (grad_h) and head-fused."""
    from deeprest_amd.ops import fused_gru_heads, fused_gru_sequence

    n_in = 7 if fused else 6
    ins = list(_inputs(shape, dtype))[:n_in]
    gen = torch.Generator().manual_seed(5)
    grad = torch.randn(*shape, O if fused else H, generator=gen).to(dtype).cuda()
    fn, ref_fn = ((fused_gru_heads, _ref_heads) if fused
                  else (fused_gru_sequence, _ref_sequence))
    out, grads = _run(fn, ins, grad, reverse)
    out_r, grads_r = _run(ref_fn, [t.float() for t in ins], grad.float(), reverse)
    _close(out, out_r, f"{shape} output")
    for name, g, g_r in zip(NAMES, grads, grads_r):
        assert torch.isfinite(g).all(), f"{name}: non-finite gradient"
        rel = ((g - g_r).abs().max() / (g_r.abs().max() + 1e-9)).item()
        print(f"{shape} {name}: max err / max magnitude {rel:.5f}")
        if shape in WAVE8:
            assert rel < 2e-2, f"{name}: relmax {rel:.4f}"
        else:
            torch.testing.assert_close(
                g, g_r, rtol=8e-2, atol=5e-2,
                msg=lambda m, n=name: f"grad mismatch for {n}: {m}")


def _kernel_results(ext, ins, lens, grad_h, grad_part, reverse):
    """Everything the chain kernels write for one set of operands: the saving
    forward (with the head phase where it exists), plain and length-aware FP8
    decode, and both backward entries on that forward's h_all / saves."""
    from deeprest_amd.ops import fused_gru_decode
    from deeprest_amd.ops.gru import _bwd_weight_images, _head_image_fwd

    xg, w_hh, b_hh, h0, gamma, beta, w_head = ins
    B, C = h0.shape[:2]
    res = {}
    if ext.gru_fwd_fuses_heads(B, C, True):
        res["h_all"], res["saves"], res["out"] = ext.gru_seq_forward(
            *ins[:6], reverse, True, False, _head_image_fwd(w_head), O)
    else:
        res["h_all"], res["saves"] = ext.gru_seq_forward(*ins[:6], reverse, True)
    with torch.no_grad():
        res["dec_out"], res["dec_last"] = fused_gru_decode(*ins, reverse=reverse)
        res["fp8_out"], res["fp8_last"] = fused_gru_decode(
            *ins, reverse=reverse, fp8=True, lengths=lens)
    w_img, w_fwd = _bwd_weight_images(w_hh)
    tail = (w_img, w_fwd, xg, gamma, beta, b_hh, h0, res["h_all"], res["saves"],
            reverse)
    res["dpre"], res["dh0"] = ext.gru_seq_backward_kernel(grad_h, *tail)
    wh_img = torch.zeros(H, 32, device=xg.device, dtype=torch.bfloat16)
    wh_img[:, :O] = w_head.t()
    res["dpre_heads"], res["dh0_heads"] = ext.gru_seq_backward_heads_kernel(
        grad_part, wh_img, *tail)
    return res


@functools.lru_cache(maxsize=None)
def _grads(shape, dtype):
    gen = torch.Generator().manual_seed(11)
    return (torch.randn(*shape, H, generator=gen).to(dtype).cuda(),
            torch.randn(*shape, O, generator=gen).to(dtype).cuda())


@functools.lru_cache(maxsize=None)
def _base_results(shape, dtype, reverse):
    from deeprest_amd.ops.native import require_native

    return _kernel_results(require_native("test"), _inputs(shape, dtype),
                           _lengths(shape), *_grads(shape, dtype), reverse)


# axis of (batch, component) in each result; None: the result has no such axis
_AXES = {"h_all": (0, 2), "saves": (0, 2), "out": (0, 2), "dec_out": (0, 2),
         "dec_last": (0, 1), "fp8_out": (0, 2), "fp8_last": (0, 1),
         "dpre": (0, 2), "dh0": (0, 1), "dpre_heads": (0, 2), "dh0_heads": (0, 1)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["components", "batch"])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_rolled_operands_give_rolled_results_bitwise(ext, shape, reverse, which, dtype):
    """Components rolled by one (gamma, beta, h0 and the upstream gradients
    along C) or the batch rolled by one: the same kernel variant, but every
    row meets another image row, wave and slot.  Every result is the rolled
    result, bit for bit."""
    xg, w_hh, b_hh, h0, gamma, beta, w_head = _inputs(shape, dtype)
    grad_h, grad_part = _grads(shape, dtype)
    lens = _lengths(shape)
    base = _base_results(shape, dtype, reverse)
    r = lambda t, d: t.roll(1, d).contiguous()
    if which == "components":
        ins = (xg, w_hh, b_hh, r(h0, 1), r(gamma, 0), r(beta, 0), w_head)
        got = _kernel_results(ext, ins, lens, r(grad_h, 2), r(grad_part, 2), reverse)
    else:
        ins = (r(xg, 0), w_hh, b_hh, r(h0, 0), gamma, beta, w_head)
        got = _kernel_results(ext, ins, r(lens, 0), r(grad_h, 0), r(grad_part, 0),
                              reverse)
    assert got.keys() == base.keys()
    for name, t in got.items():
        axis = _AXES[name][0 if which == "batch" else 1]
        assert torch.equal(t, base[name].roll(1, axis)), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [WAVE4[0], WAVE8[2]])
def test_bindings_take_natural_layout_and_leave_operands_alone(ext, shape, dtype):
    """The four entries keep taking natural-layout gamma / beta / b_hh (the
    reference comparisons above call them that way) and build their images in
    memory of their own: the operands are bit-identical after the calls."""
    ins = _inputs(shape, dtype)
    before = [t.clone() for t in ins]
    _kernel_results(ext, ins, _lengths(shape), *_grads(shape, dtype), False)
    torch.cuda.synchronize()
    for name, t, t0 in zip(NAMES, ins, before):
        assert torch.equal(t, t0), f"{name} was modified"
