"""GPU tests of ext.gru_bwd_reduce: the reductions over the GRU backward's
dpre tensor (B, T, C, 4H), pi-packed slices dr|dz|d_hhn|dn, in both forms:
"fused" (gru_reduce_fused_kernel, every row read once) and "split"
(gru_dxg_kernel + gru_dgamma_kernel).

Each output is compared with ops.gru.reference_bwd_reduce in float64 on the
same values.  The bound is derived per element from the sum it is: with N
addends a_i summed in fp32 in any order (and each product rounded once),
|error| <= N * 2^-23 * sum|a_i|; a dxg stored in bf16 adds its one rounding,
2^-8 * |ref|.  sum|a_i| comes from the same reference on the absolute values.

The last test pins dpre's slice order end to end: gradients of
ops.fused_gru_heads and ops.fused_gru_sequence in both reduce modes against
the fp32 composition, within the tiers of test_gru_heads_gpu.py.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

H = 128
LIMIT = "fused limit"            # resolved from the extension at run time
OVER = "fused limit + 1"

# (B, T, C) — each the smallest shape that reaches its case
SHAPES = [
    (1, 1, 3),       # one row, minimum C
    (2, 1, 5),       # fewer rows than one unroll group
    (3, 7, 9),       # C not a multiple of the per-thread component count
    (5, 13, 64),     # flagship C, row count ragged against unroll and slab size
    (2, 3, 63),      # C just below the flagship value
    (2, 3, LIMIT),   # the largest C the fused kernel covers
    (2, 3, OVER),    # fallback taken by auto; the fused mode raises
    (2, 3, 97),      # fallback at a large C
    (64, 60, 8),     # many workgroups flushing into the same dgamma/dbeta rows
]


@pytest.fixture(scope="module")
def ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeprest_amd.ops import native_available
    from deeprest_amd.ops.native import require_native

    if not native_available():
        pytest.fail("HIP extension not built — GPU tests must not fall back")
    return require_native("test_gru_reduce_gpu")


def _resolve(shape, ext):
    B, T, C = shape
    limit = ext.gru_reduce_fused_max_c()
    C = {LIMIT: limit, OVER: limit + 1}.get(C, C)
    return B, T, C


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """Inputs on the device, the float64 reference of the three outputs and
    the per-element sums of absolute addends; computed once per (shape,
    dtype) and shared by the modes."""
    from deeprest_amd.ops.gru import reference_bwd_reduce

    B, T, C = shape
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1000 * B + 10 * T + C)
    dpre = torch.randn(B, T, C, 4 * H, generator=gen).to(dtype).to(dev)
    gamma = (1.0 + 0.5 * torch.randn(C, 3 * H, generator=gen)).to(dtype).to(dev)
    xg = torch.randn(B, T, 3 * H, generator=gen).to(dtype).to(dev)
    ref = reference_bwd_reduce(dpre.double(), gamma.double(), xg.double())
    mag = reference_bwd_reduce(dpre.double().abs(), gamma.double().abs(),
                               xg.double().abs())
    return (dpre, gamma, xg), ref, mag


def _check(got, ref, mag, shape, dtype, what):
    B, T, C = shape
    addends = {"dxg": C, "dgamma": B * T, "dbeta4": B * T}
    for name, g, r, m in zip(addends, got, ref, mag):
        assert g.shape == r.shape, f"{what} {name}: shape {tuple(g.shape)}"
        assert torch.isfinite(g).all(), f"{what} {name}: non-finite"
        bound = addends[name] * 2.0 ** -23 * m
        if name == "dxg":
            assert g.dtype == dtype
            if dtype == torch.bfloat16:
                bound = bound + 2.0 ** -8 * r.abs()
        else:
            assert g.dtype == torch.float32
        excess = ((g.double() - r).abs() - bound).max().item()
        print(f"{what} {name}: max |err| {(g.double() - r).abs().max().item():.3e}, "
              f"max of |err| - bound {excess:.3e}")
        assert excess <= 0.0, f"{what} {name}: |err| exceeds its bound by {excess:.3e}"


@pytest.mark.parametrize("mode", ["split", "fused", "auto"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_matches_reference(ext, shape, dtype, mode):
    shape = _resolve(shape, ext)
    (dpre, gamma, xg), ref, mag = _case(shape, dtype)
    if mode == "fused" and shape[2] > ext.gru_reduce_fused_max_c():
        with pytest.raises(RuntimeError):
            ext.gru_bwd_reduce(dpre, gamma, xg, "fused")
        return
    got = ext.gru_bwd_reduce(dpre, gamma, xg, mode)
    _check(got, ref, mag, shape, dtype, f"{mode} {shape}")


def test_default_mode_is_auto_and_unknown_modes_raise(ext):
    (dpre, gamma, xg), ref, mag = _case((3, 7, 9), torch.float32)
    _check(ext.gru_bwd_reduce(dpre, gamma, xg), ref, mag, (3, 7, 9),
           torch.float32, "default")
    with pytest.raises(RuntimeError):
        ext.gru_bwd_reduce(dpre, gamma, xg, "both")
    with pytest.raises(RuntimeError):                   # gamma of another C
        ext.gru_bwd_reduce(dpre, gamma[:5].contiguous(), xg, "auto")


@pytest.mark.parametrize("mode", ["split", "fused"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 7, 9), (5, 13, 64)])
def test_no_read_past_the_last_row(ext, shape, dtype, mode):
    """dpre is the head of a larger allocation whose tail is NaN: a read past
    the last row (the fused kernel prefetches one bt ahead) would reach a sum."""
    (dpre, gamma, xg), ref, mag = _case(shape, dtype)
    n = dpre.numel()
    buf = torch.full((n + 64 * 4 * H,), float("nan"), device=dpre.device, dtype=dtype)
    buf[:n] = dpre.reshape(-1)
    head = buf[:n].view(dpre.shape)
    assert head.is_contiguous() and head.data_ptr() == buf.data_ptr()
    got = ext.gru_bwd_reduce(head, gamma, xg, mode)
    _check(got, ref, mag, shape, dtype, f"nan-tail {mode} {shape}")


# ------------------------------------------------- through the autograd ops
NAMES = ["x_gates", "w_hh", "b_hh", "h0", "gamma", "beta", "w_head"]
OP_SHAPES = [(3, 7, 5, 9), (2, 1, 3, 9), (400, 3, 64, 9)]      # (B, T, C, O)
LARGE = {(400, 3, 64, 9)}


def _op_inputs(shape):
    B, T, C, O = shape
    gen = torch.Generator().manual_seed(1000 * B + 100 * T + 10 * C + O)
    mk = lambda *s: torch.randn(*s, generator=gen) * 0.4
    ins = [mk(B, T, 3 * H), mk(3 * H, H) / H ** 0.5, mk(3 * H) * 0.2,
           mk(B, C, H), 1.0 + 0.1 * mk(C, 3 * H), 0.1 * mk(C, 3 * H),
           mk(O, H) / H ** 0.5]
    return ins, torch.randn(B, T, C, O, generator=gen), torch.randn(B, T, C, H,
                                                                   generator=gen)


def _run(fn, ins, grad, reverse):
    leaves = [t.detach().clone().requires_grad_(True) for t in ins]
    fn(*leaves, reverse=reverse).backward(grad)
    return [t.grad.detach().float() for t in leaves]


def _composed_heads(xg, w_hh, b_hh, h0, gamma, beta, w_head, reverse):
    from deeprest_amd.ops import reference_gru_sequence

    return F.linear(reference_gru_sequence(xg, w_hh, b_hh, h0, gamma, beta,
                                           reverse=reverse), w_head)


@functools.lru_cache(maxsize=None)
def _op_case(shape, reverse):
    """Device inputs and the fp32 composition's gradients for the heads op
    and the sequence op, once per (shape, direction)."""
    from deeprest_amd.ops import reference_gru_sequence

    dev = torch.device("cuda:0")
    ins, grad_o, grad_h = _op_inputs(shape)
    ins = [t.to(dev) for t in ins]
    grad_o, grad_h = grad_o.to(dev), grad_h.to(dev)
    ref_heads = _run(_composed_heads, ins, grad_o, reverse)
    ref_seq = _run(reference_gru_sequence, ins[:6], grad_h, reverse)
    return ins, grad_o, grad_h, ref_heads, ref_seq


def _check_grads(grads, refs, names, large, what):
    for name, g, g_r in zip(names, grads, refs):
        assert torch.isfinite(g).all(), f"{what} {name}: non-finite gradient"
        if large:
            err = (g - g_r).abs().max()
            scale = g_r.abs().max() + 1e-9
            assert err / scale < 2e-2, f"{what} {name}: relmax {(err / scale).item():.4f}"
        else:
            torch.testing.assert_close(
                g, g_r, rtol=8e-2, atol=5e-2,
                msg=lambda m, n=name: f"{what} grad mismatch for {n}: {m}")


@pytest.mark.parametrize("mode", ["fused", "split"])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", OP_SHAPES)
def test_ops_gradients_in_both_modes(ext, monkeypatch, shape, reverse, mode):
    from deeprest_amd.ops import fused_gru_heads, fused_gru_sequence
    from deeprest_amd.ops import gru as gru_mod

    seen = []
    real = ext.gru_bwd_reduce

    class Spy:
        """The extension, recording the mode the reductions were asked for."""

        def __getattr__(self, name):
            return getattr(ext, name)

        def gru_bwd_reduce(self, dpre, gamma, xg, mode="auto"):
            seen.append(mode)
            return real(dpre, gamma, xg, mode)

    monkeypatch.setattr(gru_mod, "REDUCE_MODE", mode)
    monkeypatch.setattr(gru_mod, "require_native", lambda what: Spy())
    ins, grad_o, grad_h, ref_heads, ref_seq = _op_case(shape, reverse)
    large = shape in LARGE
    _check_grads(_run(fused_gru_heads, ins, grad_o, reverse), ref_heads, NAMES,
                 large, f"heads {mode} {shape}")
    _check_grads(_run(fused_gru_sequence, ins[:6], grad_h, reverse), ref_seq,
                 NAMES[:6], large, f"sequence {mode} {shape}")
    assert seen == [mode, mode]
